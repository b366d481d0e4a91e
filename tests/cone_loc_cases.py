"""Inputs and raw calls shared by tests/test_cone_loc_cpu.py and tests/test_cone_loc_gpu.py: the cone map of fsg2019
(tests/golden/tracks/cones.npz), the poses of the sense tests, direct ctypes calls of fsaempc_cl_cone_sense_batch_device and
fsaempc_cl_estimate_cones_batch_device on numpy inputs, and the list of their refusals (decided before any launch, so the same list runs
on host buffers without a device)."""
import ctypes as C
import os

import numpy as np

import sensors_cases as sc
import sensors_numpy as sn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT, B, N, SEED = sc.DT, sc.B, sc.N, sc.SEED
SENSOR = dict(r_min=0.5, r_max=15.0, fov=2 * np.pi / 3, sigma=(0.05, 0.01), p_detect=1.0, k_max=16)
R_CONE = np.array([0.05 ** 2, 0.01 ** 2])
POSE_SEED = 12
MARGIN = 1e-9


def cone_map(name="fsg2019"):
    """(left (K, 2), right (K, 2)) of a track's cones"""
    with np.load(os.path.join(ROOT, "tests", "golden", "tracks", "cones.npz")) as z:
        return np.ascontiguousarray(z[name + "_left"], dtype=np.float64), np.ascontiguousarray(z[name + "_right"], dtype=np.float64)


def poses(otr, batch=B, seed=POSE_SEED):
    """(batch, 7) Cartesian states of cars spread over the track: |n| <= 0.5 m, |mu| <= 0.2 rad off the centre line"""
    rng = np.random.default_rng(seed)
    cart = np.zeros((batch, 7))
    for b in range(batch):
        x = np.array([otr.L * (b + rng.uniform(0.1, 0.9)) / batch, rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2), 8.0, 0.0])
        hv = sn.h_values(otr, x)
        cart[b] = [hv[0], hv[1], hv[2], 8.0, 0.0, 0.0, 0.0]
    return cart


def synthetic_map(cart, per_side=512, seed=3):
    """A map of 512 cones per side (every lane of the sense kernel strides 16 times): a ring of 5 .. 25 m around every third car's
    position and a scatter over the track's bounding box"""
    rng = np.random.default_rng(seed)
    K = 2 * per_side
    pts = np.zeros((K, 2))
    lo, hi = cart[:, :2].min(axis=0) - 20.0, cart[:, :2].max(axis=0) + 20.0
    pts[:] = rng.uniform(lo, hi, (K, 2))
    near = K // 2
    c = cart[rng.integers(0, len(cart), near), :2]
    rad, ang = rng.uniform(1.0, 25.0, near), rng.uniform(0, 2 * np.pi, near)
    pts[:near] = c + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    pts = pts[rng.permutation(K)]
    return np.ascontiguousarray(pts[:per_side]), np.ascontiguousarray(pts[per_side:])


def margins_ok(cand, r_min, r_max, fov, margin=MARGIN):
    """No candidate within `margin` of the view's edges, and any two candidates of a car either at identical ranges (the same position
    twice) or more than `margin` apart"""
    for car in cand:
        rho = np.array([c[1] for c in car]); beta = np.array([c[2] for c in car])
        if len(rho) == 0:
            continue
        if min(np.abs(rho - r_min).min(), np.abs(rho - r_max).min(), np.abs(np.abs(beta) - fov / 2).min()) <= margin:
            return False
        d = np.abs(rho[:, None] - rho[None, :])
        if ((d > 0) & (d <= margin)).any():
            return False
    return True


class Direct(sc.Direct):
    """sensors_cases.Direct plus the two entries of 6t on numpy inputs"""

    def _map(self, left, right):
        from fsae_mpc_amd import _lib
        left, right = np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)
        tl, tr_ = self.dev(left), self.dev(right)
        p = lambda t: None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())
        return _lib.ConeMaps(p(tl), p(tr_), left.shape[-2], right.shape[-2], 1 if left.ndim == 3 else 0), (tl, tr_)

    def cone_sense(self, cart, left, right, *, r_min, r_max, fov, sigma, p_detect, k_max, seed=SEED, id0=0, step=0, finished=None):
        """-> dict n, seen, ids, z (numpy)"""
        from fsae_mpc_amd import _lib
        torch, nb = self.torch, len(cart)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        maps, keep = self._map(left, right)
        tc, tf = self.dev(cart), self.dev(finished, torch.int32)
        n = torch.full((nb,), -7, dtype=torch.int32, device=self.device); seen = torch.full((nb,), -7, dtype=torch.int32, device=self.device)
        ids = torch.full((nb, k_max), -7, dtype=torch.int32, device=self.device)
        z = torch.full((nb, k_max, 2), -777.0, dtype=torch.float64, device=self.device)
        sens = _lib.ClConeSensor(C.pointer(maps), r_min, r_max, fov, sigma[0], sigma[1], p_detect, k_max, seed, id0)
        rc = self.fm.lib().fsaempc_cl_cone_sense_batch_device(nb, C.byref(sens), step, p(tc), p(tf), p(n), p(seen), p(ids), p(z), None)
        _lib.check(rc, "fsaempc_cl_cone_sense_batch_device")
        torch.cuda.synchronize()
        return dict(n=n.cpu().numpy(), seen=seen.cpu().numpy(), ids=ids.cpu().numpy(), z=z.cpu().numpy())

    def estimate_cones(self, *, y, x_proj, u_prev, q, r, p0, map_left, map_right, cone_n, cone_id, cone_z, r_cone=R_CONE, L=0.0, finished=None, est_x=None,
                       est_P=None, est_count=None, want=True):
        """-> the dict of sensors_cases.Direct.estimate plus cone_innov, rows_used and (want) G_out"""
        from fsae_mpc_amd import _lib
        torch, nb, nx, dev = self.torch, self.batch, self.nx, self.dev
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
        tq, tr_, tp0, ty, txp, tu, tfin = dev(q), dev(r), dev(p0), dev(y), dev(x_proj), dev(u_prev), dev(finished, torch.int32)
        est = _lib.ClEstimator(p(tq), 1 if q.ndim == 2 else 0, p(tr_), 1 if r.ndim == 2 else 0, p(tp0), float(L))
        ex = dev(est_x) if est_x is not None else torch.full((nb, nx), 123.0, dtype=torch.float64, device=self.device)
        eP = dev(est_P) if est_P is not None else torch.full((nb, nx, nx), 123.0, dtype=torch.float64, device=self.device)
        ec = dev(est_count, torch.int32) if est_count is not None else torch.zeros((nb, 2), dtype=torch.int32, device=self.device)
        f64 = lambda *s: torch.full(s, -777.0, dtype=torch.float64, device=self.device)
        x0e, inn, nis = f64(nb, nx), f64(nb, nx), f64(nb)
        Fo, xpr, Ho = (f64(nb, nx, nx), f64(nb, nx), f64(nb, nx, nx)) if want else (None, None, None)
        cone_id = np.ascontiguousarray(cone_id, dtype=np.int32)
        k_max = cone_id.shape[1]
        maps, keep = self._map(map_left, map_right)
        tn, ti, tz = dev(np.asarray(cone_n), torch.int32), dev(cone_id, torch.int32), dev(np.asarray(cone_z, dtype=np.float64))
        ci, ru = f64(nb, k_max, 2), torch.full((nb,), -7, dtype=torch.int32, device=self.device)
        Go = f64(nb, k_max, 2, 3) if want else None
        rc_ = (C.c_double * 2)(float(r_cone[0]), float(r_cone[1]))
        mpc = self.mpc
        rc = self.fm.lib().fsaempc_cl_estimate_cones_batch_device(C.byref(mpc.desc), C.byref(mpc.sp), mpc.params.ref() if mpc.params is not None else None,
                                                                  C.byref(est), p(ty), p(txp), p(tu), int(np.prod(np.shape(u_prev)[1:])), p(tfin), p(ex), p(eP),
                                                                  p(ec), p(x0e), p(inn), p(nis), p(Fo), p(xpr), p(Ho), C.byref(maps), k_max, rc_, p(tn), p(ti),
                                                                  p(tz), p(ci), p(ru), p(Go), None)
        _lib.check(rc, "fsaempc_cl_estimate_cones_batch_device")
        torch.cuda.synchronize()
        g = lambda t: None if t is None else t.cpu().numpy()
        return dict(est_x=g(ex), est_P=g(eP), est_count=g(ec), x0_est=g(x0e), innov=g(inn), nis=g(nis), F_out=g(Fo), x_prior=g(xpr), H_out=g(Ho),
                    cone_innov=g(ci), rows_used=g(ru), G_out=g(Go))


def check_abi_refusals(device):
    """Every refusal of the two entries returns its code with a text that names the argument and leaves the buffers untouched; batch 0
    succeeds without a launch."""
    import torch
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    err = lambda: L.fsaempc_last_error()
    ARG = -1
    assert L.fsaempc_cl_cone_sense_batch_device(1, None, 0, None, None, None, None, None, None, None) == ARG and b"sensor" in err()
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=device)
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=device)
    nb, K, kc = 3, 4, 6
    left, right = f64(kc, 2), f64(kc, 2)

    def cones(n_left=kc, n_right=kc, lp=True, rp=True, per=0):
        return _lib.ConeMaps(p(left) if lp else None, p(right) if rp else None, n_left, n_right, per)

    # ---- sense ----
    names = ("cart", "finished", "cone_n", "cone_seen", "cone_id", "cone_z")
    bufs = dict(cart=f64(nb, 7), finished=torch.zeros(nb, dtype=torch.int32, device=device), cone_n=i32(nb), cone_seen=i32(nb), cone_id=i32(nb, K),
                cone_z=f64(nb, K, 2))
    big = f64(4 * nb * K)

    def sense(batch=nb, step=0, null=(), swap=None, truth=True, maps=None, **kw):
        m = maps if maps is not None else cones()
        v = dict(r_min=0.5, r_max=15.0, fov=2.0, sigma_range=0.05, sigma_bearing=0.01, p_detect=1.0, k_max=K, seed=1, id0=0)
        v.update(kw)
        se = _lib.ClConeSensor(C.pointer(m) if truth else None, v["r_min"], v["r_max"], v["fov"], v["sigma_range"], v["sigma_bearing"], v["p_detect"],
                               v["k_max"], v["seed"], v["id0"])
        ptr = {k: (None if k in null else p(bufs[k])) for k in names}
        ptr.update(swap or {})
        return L.fsaempc_cl_cone_sense_batch_device(batch, C.byref(se), step, *[ptr[k] for k in names], None)
    inf, nan = float("inf"), float("nan")
    assert sense(batch=0) == 0 and sense(batch=0, null=("finished",)) == 0      # nothing to launch
    assert sense(batch=-1) == ARG and b"batch" in err()
    assert sense(truth=False) == ARG and b"null" in err() and b"truth" in err()
    for k in ("cart", "cone_n", "cone_seen", "cone_id", "cone_z"):
        assert sense(null=(k,)) == ARG and b"null" in err() and k.encode() in err(), k
    for k_max in (0, -1, 17):
        assert sense(k_max=k_max) == ARG and b"k_max" in err(), k_max
    for kw in (dict(r_min=0.0), dict(r_min=-1.0), dict(r_min=nan), dict(r_min=15.0), dict(r_min=16.0), dict(r_max=inf), dict(r_max=nan)):
        assert sense(**kw) == ARG and b"r_min" in err(), kw
    for fov in (0.0, -1.0, 6.3, nan, inf):
        assert sense(fov=fov) == ARG and b"fov" in err(), fov
    assert sense(fov=2 * np.pi, batch=0) == 0
    for k in ("sigma_range", "sigma_bearing"):
        for v in (-1e-9, nan):
            assert sense(**{k: v}) == ARG and k.encode() in err(), (k, v)
    for v in (-0.1, 1.1, nan):
        assert sense(p_detect=v) == ARG and b"p_detect" in err(), v
    assert sense(id0=-1) == ARG and b"id0" in err()
    for step in (-1, 2 ** 32, 2 ** 40):
        assert sense(step=step) == ARG and b"step" in err(), step
    assert sense(maps=cones(0, 0)) == ARG and b"no cones" in err()
    assert sense(maps=cones(-1, 2)) == ARG and b"negative" in err()
    assert sense(maps=cones(lp=False)) == ARG and b"null" in err()
    assert sense(maps=cones(rp=False)) == ARG and b"null" in err()
    assert sense(maps=cones(0, kc, lp=False), batch=0) == 0                      # (an empty side needs no pointer)
    assert sense(maps=cones(513, 2)) == -2 and sense(maps=cones(2, 513)) == -2 and b"FSAEMPC_CONES_MAX" in err()
    assert sense(swap=dict(cone_n=p(bufs["cone_seen"]))) == ARG and b"overlap" in err()
    assert sense(swap=dict(cone_z=p(bufs["cart"]))) == ARG and b"overlap" in err()
    assert sense(swap=dict(cone_z=p(left))) == ARG and b"overlap" in err()
    assert sense(swap=dict(cone_id=C.c_void_p(big.data_ptr()), cone_z=C.c_void_p(big.data_ptr() + 4 * (nb * K - 1)))) == ARG and b"overlap" in err()
    assert all(bool((bufs[k] == 7).all()) for k in names if k != "finished") and bool((big == 7).all()) and bool((left == 7).all())

    # ---- estimate ----
    hor = 4
    for nx in (5, 7):
        model = 0 if nx == 5 else 1
        table = torch.zeros(8 * 4, dtype=torch.float64, device=device)     # (a spline table is only pointed at: nothing is launched)
        sp = _lib.Spline(4, 1.0, p(table), p(table))
        names = ("y", "x_proj", "u_prev", "finished", "est_x", "est_P", "est_count", "x0_est", "innov", "nis", "F_out", "x_prior", "H_out",
                 "cone_n", "cone_id", "cone_z", "cone_innov", "rows_used", "G_out")
        bufs = dict(y=f64(nb, nx), x_proj=f64(nb, nx), u_prev=f64(nb, hor, 2), finished=torch.zeros(nb, dtype=torch.int32, device=device),
                    est_x=f64(nb, nx), est_P=f64(nb, nx, nx), est_count=i32(nb, 2), x0_est=f64(nb, nx), innov=f64(nb, nx), nis=f64(nb),
                    F_out=f64(nb, nx, nx), x_prior=f64(nb, nx), H_out=f64(nb, nx, nx), cone_n=i32(nb), cone_id=i32(nb, K), cone_z=f64(nb, K, 2),
                    cone_innov=f64(nb, K, 2), rows_used=i32(nb), G_out=f64(nb, K, 2, 3))
        var = dict(q=f64(nx), r=f64(nx), p0=f64(nx))
        big = f64(nb * K * 8 + nb * nx)

        def call(model_=model, N_=hor, batch=nb, dt=DT, integ=-1, Lap=0.0, stride=2 * hor, null=(), swap=None, desc=True, spl=True, est=True, maps=True,
                 m=None, k_max=K, rcone=True):
            d = _lib.LtvDesc(model_, N_, batch, dt, integ)
            v = {k: (None if k in null else p(var[k])) for k in var}
            e = _lib.ClEstimator(v["q"], 0, v["r"], 0, v["p0"], Lap)
            ptr = {k: (None if k in null else p(bufs[k])) for k in names}
            ptr.update(swap or {})
            a = [ptr[k] for k in names]
            mm = m if m is not None else cones()
            return L.fsaempc_cl_estimate_cones_batch_device(C.byref(d) if desc else None, C.byref(sp) if spl else None, None, C.byref(e) if est else None,
                                                            a[0], a[1], a[2], stride, *a[3:13], C.byref(mm) if maps else None, k_max,
                                                            (C.c_double * 2)(0.01, 0.01) if rcone else None, *a[13:], None)
        assert call(batch=0) == 0 and call(batch=0, null=("finished", "F_out", "x_prior", "H_out", "G_out")) == 0      # nothing to launch
        for kw in (dict(desc=False), dict(spl=False)):                      # everything the 6s entry refuses
            assert call(**kw) == ARG and b"null" in err(), kw
        assert call(est=False) == ARG and b"null" in err() and b"est" in err()
        for k in ("q", "r", "p0", "y", "x_proj", "u_prev", "est_x", "est_P", "est_count", "x0_est", "innov", "nis"):
            assert call(null=(k,)) == ARG and b"null" in err() and k.encode() in err(), k
        assert call(model_=2) == ARG and b"model" in err()
        for kw in (dict(N_=0), dict(batch=-1), dict(dt=0.0), dict(integ=3), dict(integ=-2)):
            assert call(**kw) == ARG and len(err()) > 0, kw
        for Lap in (-1.0, inf, nan):
            assert call(Lap=Lap) == ARG and b"L must" in err(), Lap
        for stride in (1, 0, -4):
            assert call(stride=stride) == ARG and b"u_stride" in err(), stride
        assert call(maps=False) == ARG and b"null" in err() and b"map" in err()          # the cone arguments
        assert call(rcone=False) == ARG and b"null" in err() and b"r_cone" in err()
        for k in ("cone_n", "cone_id", "cone_z", "cone_innov", "rows_used"):
            assert call(null=(k,)) == ARG and b"null" in err() and k.encode() in err(), k
        for k_max in (0, -3, 17):
            assert call(k_max=k_max) == ARG and b"k_max" in err(), k_max
        assert call(m=cones(0, 0)) == ARG and b"no cones" in err()
        assert call(m=cones(2, -2)) == ARG and b"negative" in err()
        assert call(m=cones(rp=False)) == ARG and b"null" in err()
        assert call(m=cones(600, 2)) == -2 and b"FSAEMPC_CONES_MAX" in err()
        assert call(swap=dict(x0_est=p(bufs["est_x"]))) == ARG and b"overlap" in err()
        assert call(swap=dict(cone_innov=p(bufs["cone_z"]))) == ARG and b"overlap" in err()
        assert call(swap=dict(G_out=p(bufs["H_out"]))) == ARG and b"overlap" in err()
        assert call(swap=dict(rows_used=p(bufs["cone_n"]))) == ARG and b"overlap" in err()
        assert call(swap=dict(cone_innov=p(left))) == ARG and b"overlap" in err()
        assert call(swap=dict(innov=p(bufs["cone_id"]))) == ARG and b"overlap" in err()
        assert call(swap=dict(G_out=C.c_void_p(big.data_ptr()), est_x=C.c_void_p(big.data_ptr() + 8 * (nb * K * 6 - 1)))) == ARG and b"overlap" in err()
        assert all(bool((bufs[k] == 7).all()) for k in names if k != "finished") and bool((big == 7).all()) and bool((right == 7).all())


# ---- localising without a pose measurement: the synthetic drive of sensors_cases.gain_drive ----
LOC_OFFSET = np.array([0.0, 0.3, 0.05, 0.0, 0.0])       # the first prior: 0.3 m off in n, 0.05 rad off in mu
LOC_R = np.array([np.inf, np.inf, np.inf, sc.GAIN_SIGMA[3] ** 2, sc.GAIN_SIGMA[4] ** 2])
LOC_P0 = np.array([0.05 ** 2, 0.3 ** 2, 0.05 ** 2, sc.GAIN_SIGMA[3] ** 2, sc.GAIN_SIGMA[4] ** 2])     # what the first prior is good for
LOC_ID0 = 500
_LOC = {}


def loc_carts(otr, truth_k):
    """The Cartesian states of the drive's cars at their true states of one period"""
    cart = np.zeros((len(truth_k), 7))
    for c, x in enumerate(truth_k):
        hv = sn.h_values(otr, x)
        cart[c] = [hv[0], hv[1], hv[2], hv[3], 0.0, 0.0, hv[4]]
    return cart


def loc_figures(truth, with_cones, without):
    """RMS errors in n and mu over periods GAIN_FROM .. of the two filters, and their ratios"""
    sl = slice(sc.GAIN_FROM, None)
    rms = lambda a, i: float(np.sqrt(np.mean((a[sl, :, i] - truth[sl, :, i]) ** 2)))
    rn, rmu = (rms(with_cones, 1), rms(without, 1)), (rms(with_cones, 2), rms(without, 2))
    return dict(rms_n=rn, rms_mu=rmu, ratio=(rn[0] / rn[1], rmu[0] / rmu[1]))


def localise_restated(orc, otr):
    """The drive through cone_loc_numpy.sense and cone_loc_numpy.period (F by differences of param_numpy.psi), with and without the cone
    rows; computed once.  dict: the figures of loc_figures, x_est of both runs, resets and the least number of cones a car kept."""
    import cone_loc_numpy as cn
    import estimator_numpy as en
    if "res" in _LOC:
        return _LOC["res"]
    d = sc.gain_drive(orc, otr)
    left, right = cone_map()
    K, Cn, nx = d["truth"].shape
    predict = lambda x, u: (sc.pn.psi(d["block"], orc, sc.GAIN_MODEL, otr, x, u, sc.DT, sc.GAIN_INTEG),
                            en.psi_jacobian(d["block"], orc, sc.GAIN_MODEL, otr, x, u, sc.DT, sc.GAIN_INTEG)[0])
    lin = lambda x: sn.linearise(otr, x)
    est = {True: np.zeros((K, Cn, nx)), False: np.zeros((K, Cn, nx))}
    st = {(w, c): dict(est_x=np.zeros(nx), est_P=np.zeros((nx, nx)), count=(0, 0)) for w in (True, False) for c in range(Cn)}
    least = 99
    for k in range(K):
        obs = cn.sense(left, right, loc_carts(otr, d["truth"][k]), LOC_ID0, k, **dict(SENSOR, seed=SEED))
        least = min(least, int(obs["n"].min()))
        for c in range(Cn):
            for w in (True, False):
                cones = cn.cone_list(left, right, obs["n"][c] if w else 0, obs["ids"][c], obs["z"][c])
                s = st[(w, c)]
                s = cn.period(s["est_x"], s["est_P"], s["count"], d["y"][k, c], d["truth"][k, c] + LOC_OFFSET, d["u"][k - 1, c] if k else np.zeros(2), 0,
                              sc.GAIN_Q, LOC_R, LOC_P0, 0.0, predict, lin, cones, R_CONE)
                st[(w, c)] = s
                est[w][k, c] = s["x0_est"]
    res = loc_figures(d["truth"], est[True], est[False])
    res.update(x_est=est[True], x_est_without=est[False], resets=sum(s["count"][1] for s in st.values()), cones_min=least, drive=d)
    _LOC["res"] = res
    return res
