"""Inputs and raw calls shared by tests/test_sensors_cpu.py and tests/test_sensors_gpu.py: direct ctypes calls of
fsaempc_cl_sense_batch_device and fsaempc_cl_estimate_cart_batch_device on numpy inputs, the list of their refusals (decided before any
launch, so the same list runs on host buffers without a device) and the synthetic drive of the filtering-gain tests."""
import ctypes as C

import numpy as np

import param_numpy as pn
import sensors_numpy as sn

DT = 0.05
B, N = 70, 10      # nine wavefronts of 8 cars, the last group of lanes partial
SEED = 2 ** 40 + 11
SIGMA = {0: np.array([0.05, 0.05, 0.01, 0.1, 0.005]), 1: np.array([0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005])}


class Direct:
    """The two entries on numpy inputs for one (model, batch, params, integrator): the descriptor, spline and block of an LtvBatch."""

    def __init__(self, fm, torch, tr, model, batch, params=None, integrator=-1, horizon=N, device="cuda"):
        self.fm, self.torch, self.device, self.batch, self.model = fm, torch, device, batch, model
        self.nx = sn.nx_of(model)
        self.mpc = fm.LtvBatch(model, horizon, DT, tr, batch, integrator=integrator, params=params, device=device)

    def dev(self, a, dt=None):
        torch = self.torch
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt or torch.float64, device=self.device)

    def sense(self, cart, x0_true, sigma, *, seed=SEED, id0=0, step=0, finished=None, proj_lost=None):
        """-> dict y, x_proj, proj_lost (numpy)"""
        from fsae_mpc_amd import _lib
        torch, nb, nx = self.torch, self.batch, self.nx
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        sg = self.dev(np.asarray(sigma, dtype=np.float64))
        tc, tx, tf = self.dev(cart), self.dev(x0_true), self.dev(finished, torch.int32)
        y = torch.full((nb, nx), -777.0, dtype=torch.float64, device=self.device)
        xp = torch.full((nb, nx), -777.0, dtype=torch.float64, device=self.device)
        pl = self.dev(proj_lost, torch.int32) if proj_lost is not None else torch.zeros(nb, dtype=torch.int32, device=self.device)
        sens = _lib.ClSensors(p(sg), 1 if sg.dim() == 2 else 0, seed, id0)
        rc = self.fm.lib().fsaempc_cl_sense_batch_device(C.byref(self.mpc.desc), C.byref(self.mpc.sp), C.byref(sens), step, p(tc), p(tx), p(tf), p(y), p(xp),
                                                         p(pl), None)
        _lib.check(rc, "fsaempc_cl_sense_batch_device")
        torch.cuda.synchronize()
        return dict(y=y.cpu().numpy(), x_proj=xp.cpu().numpy(), proj_lost=pl.cpu().numpy())

    def estimate(self, *, y, x_proj, u_prev, q, r, p0, L=0.0, finished=None, est_x=None, est_P=None, est_count=None, want=True):
        """-> dict est_x, est_P, est_count, x0_est, innov, nis and (want) F_out, x_prior, H_out (numpy).  u_prev: (batch, horizon, 2) plans
        (stage 1 is read) or (batch, 2)."""
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
        mpc = self.mpc
        rc = self.fm.lib().fsaempc_cl_estimate_cart_batch_device(C.byref(mpc.desc), C.byref(mpc.sp), mpc.params.ref() if mpc.params is not None else None,
                                                                 C.byref(est), p(ty), p(txp), p(tu), int(np.prod(np.shape(u_prev)[1:])), p(tfin), p(ex), p(eP),
                                                                 p(ec), p(x0e), p(inn), p(nis), p(Fo), p(xpr), p(Ho), None)
        _lib.check(rc, "fsaempc_cl_estimate_cart_batch_device")
        torch.cuda.synchronize()
        g = lambda t: None if t is None else t.cpu().numpy()
        return dict(est_x=g(ex), est_P=g(eP), est_count=g(ec), x0_est=g(x0e), innov=g(inn), nis=g(nis), F_out=g(Fo), x_prior=g(xpr), H_out=g(Ho))


def check_abi_refusals(device):
    """Every FSAEMPC_ERR_ARG case of the two entries returns that code with a text that names the argument and leaves the buffers
    untouched; batch 0 succeeds without a launch."""
    import torch
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    err = lambda: L.fsaempc_last_error()
    nb, hor = 3, 4
    for nx in (5, 7):
        model = 0 if nx == 5 else 1
        table = torch.zeros(8 * 4, dtype=torch.float64, device=device)     # (a spline table is only pointed at: nothing is launched)
        sp = _lib.Spline(4, 1.0, p(table), p(table))
        f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=device)

        # ---- sense ----
        names = ("cart", "x0_true", "finished", "y", "x_proj", "proj_lost")
        bufs = dict(cart=f64(nb, 7), x0_true=f64(nb, nx), finished=torch.zeros(nb, dtype=torch.int32, device=device), y=f64(nb, nx), x_proj=f64(nb, nx),
                    proj_lost=i32(nb))
        sigma = f64(nx)
        big = f64(2 * nb * nx)

        def sense(model_=model, N_=hor, batch=nb, dt=DT, integ=-1, id0=0, step=0, null=(), swap=None, desc=True, spl=True, sens=True, sig=True):
            d = _lib.LtvDesc(model_, N_, batch, dt, integ)
            se = _lib.ClSensors(p(sigma) if sig else None, 0, 1, id0)
            ptr = {k: (None if k in null else p(bufs[k])) for k in names}
            ptr.update(swap or {})
            return L.fsaempc_cl_sense_batch_device(C.byref(d) if desc else None, C.byref(sp) if spl else None, C.byref(se) if sens else None, step,
                                                   *[ptr[k] for k in names], None)
        assert sense(batch=0) == 0 and sense(batch=0, null=("finished",)) == 0      # nothing to launch
        for kw in (dict(desc=False), dict(spl=False)):
            assert sense(**kw) == -1 and b"null" in err(), kw
        assert sense(sens=False) == -1 and b"null" in err() and b"sens" in err()
        assert sense(sig=False) == -1 and b"null" in err() and b"sigma" in err()
        for k in ("cart", "x0_true", "y", "x_proj", "proj_lost"):
            assert sense(null=(k,)) == -1 and b"null" in err() and k.encode() in err(), k
        assert sense(model_=2) == -1 and b"model" in err()
        for kw in (dict(N_=0), dict(batch=-1), dict(dt=0.0), dict(integ=3), dict(integ=-2)):
            assert sense(**kw) == -1 and len(err()) > 0, kw
        for step in (-1, 2 ** 32, 2 ** 40):
            assert sense(step=step) == -1 and b"step" in err(), step
        assert sense(id0=-1) == -1 and b"id0" in err()
        assert sense(swap=dict(y=p(bufs["x_proj"]))) == -1 and b"overlap" in err()
        assert sense(swap=dict(y=C.c_void_p(big.data_ptr()), x_proj=C.c_void_p(big.data_ptr() + 8 * (nb * nx - 1)))) == -1 and b"overlap" in err()
        assert sense(swap=dict(x_proj=p(bufs["x0_true"]))) == -1 and b"overlap" in err()
        assert sense(swap=dict(y=p(bufs["cart"]))) == -1 and b"overlap" in err()
        assert sense(swap=dict(y=p(sigma))) == -1 and b"overlap" in err()
        assert all(bool((bufs[k] == 7).all()) for k in names if k != "finished") and bool((big == 7).all())

        # ---- estimate ----
        names = ("y", "x_proj", "u_prev", "finished", "est_x", "est_P", "est_count", "x0_est", "innov", "nis", "F_out", "x_prior", "H_out")
        big = f64(nb * nx * nx + nb * nx)                                  # (one allocation two outputs can share)
        bufs = dict(y=f64(nb, nx), x_proj=f64(nb, nx), u_prev=f64(nb, hor, 2), finished=torch.zeros(nb, dtype=torch.int32, device=device),
                    est_x=f64(nb, nx), est_P=f64(nb, nx, nx), est_count=i32(nb, 2), x0_est=f64(nb, nx), innov=f64(nb, nx), nis=f64(nb),
                    F_out=f64(nb, nx, nx), x_prior=f64(nb, nx), H_out=f64(nb, nx, nx))
        var = dict(q=f64(nx), r=f64(nx), p0=f64(nx))

        def call(model_=model, N_=hor, batch=nb, dt=DT, integ=-1, Lap=0.0, stride=2 * hor, null=(), swap=None, desc=True, spl=True, est=True):
            d = _lib.LtvDesc(model_, N_, batch, dt, integ)
            v = {k: (None if k in null else p(var[k])) for k in var}
            e = _lib.ClEstimator(v["q"], 0, v["r"], 0, v["p0"], Lap)
            ptr = {k: (None if k in null else p(bufs[k])) for k in names}
            ptr.update(swap or {})
            a = [ptr[k] for k in names]
            return L.fsaempc_cl_estimate_cart_batch_device(C.byref(d) if desc else None, C.byref(sp) if spl else None, None, C.byref(e) if est else None,
                                                           a[0], a[1], a[2], stride, *a[3:], None)
        assert call(batch=0) == 0 and call(batch=0, null=("finished", "F_out", "x_prior", "H_out")) == 0      # nothing to launch
        for kw in (dict(desc=False), dict(spl=False)):
            assert call(**kw) == -1 and b"null" in err(), kw
        assert call(est=False) == -1 and b"null" in err() and b"est" in err()
        for k in ("q", "r", "p0", "y", "x_proj", "u_prev", "est_x", "est_P", "est_count", "x0_est", "innov", "nis"):
            assert call(null=(k,)) == -1 and b"null" in err() and k.encode() in err(), k
        assert call(model_=2) == -1 and b"model" in err()
        for kw in (dict(N_=0), dict(batch=-1), dict(dt=0.0), dict(integ=3), dict(integ=-2)):
            assert call(**kw) == -1 and len(err()) > 0, kw
        for Lap in (-1.0, float("inf"), float("nan")):
            assert call(Lap=Lap) == -1 and b"L must" in err(), Lap
        for stride in (1, 0, -4):
            assert call(stride=stride) == -1 and b"u_stride" in err(), stride
        assert call(swap=dict(x0_est=p(bufs["est_x"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(H_out=p(bufs["F_out"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(innov=p(bufs["x_prior"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(est_P=C.c_void_p(big.data_ptr()), est_x=C.c_void_p(big.data_ptr() + 8 * (nb * nx * nx - 1)))) == -1 and b"overlap" in err()
        assert call(swap=dict(x0_est=p(bufs["y"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(est_x=p(bufs["x_proj"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(nis=p(var["p0"]))) == -1 and b"overlap" in err()
        assert all(bool((bufs[k] == 7).all()) for k in names if k != "finished") and bool((big == 7).all())


# ---- the synthetic drive of the filtering-gain tests ----
GAIN_MODEL, GAIN_CARS, GAIN_PERIODS, GAIN_FROM = 0, 8, 30, 10
GAIN_SIGMA = SIGMA[0]
GAIN_Q = 1e-4 * SIGMA[0] ** 2      # the truth follows the filter's own model exactly: the process noise only keeps P from collapsing
GAIN_INTEG = 1                     # RK2, the kinematic default


def gain_drive(orc, otr):
    """Truth rolled with param_numpy.psi (kinematic, the default block) under a steering law that keeps the car near the centre line
    (the wheel follows atan(wheelbase * kappa) a little ahead, less a share of n and mu), exact measurements h(truth) and numpy noise on
    them.  dict: truth (K, C, nx), y (K, C, nx) noisy measurements in the sensor layout, u (K, C, 2): u[k] drives truth[k] -> truth[k + 1]."""
    from dual_numpy import default_block
    P = default_block(GAIN_MODEL)
    wheelbase = pn.g(P, "LF") + pn.g(P, "LR")
    rng = np.random.default_rng(606)
    nx = 5
    x = np.zeros((GAIN_CARS, nx))
    x[:, 0] = 10.0 + 31.0 * np.arange(GAIN_CARS); x[:, 1] = 0.1 * np.cos(np.arange(GAIN_CARS)); x[:, 3] = 5.0 + 0.5 * np.arange(GAIN_CARS)
    wheel = lambda xc: np.arctan(wheelbase * orc.kappa(otr, xc[0] + 0.1 * xc[3])) - 0.3 * xc[1] - 1.0 * xc[2]
    x[:, 4] = [wheel(x[c]) for c in range(GAIN_CARS)]
    truth, ys, us = [], [], []
    for k in range(GAIN_PERIODS):
        truth.append(x.copy())
        ys.append(np.stack([sn.h_values(otr, x[c]) for c in range(GAIN_CARS)]) + GAIN_SIGMA * rng.standard_normal((GAIN_CARS, nx)))
        u = np.stack([np.array([1.0 * np.sin(0.3 * k + c), float(np.clip((wheel(x[c]) - x[c, 4]) / (2 * DT), -2.0, 2.0))]) for c in range(GAIN_CARS)])
        us.append(u)
        x = np.stack([pn.psi(P, orc, GAIN_MODEL, otr, x[c], u[c], DT, GAIN_INTEG) for c in range(GAIN_CARS)])
    return dict(truth=np.stack(truth), y=np.stack(ys), u=np.stack(us), block=P)


def gain_ratio(truth, x_proj, x_est):
    """RMS error of the estimate over that of the projection in n and in mu, over the periods GAIN_FROM .. and all cars -> (ratio_n, ratio_mu)"""
    sl = slice(GAIN_FROM, None)
    rms = lambda a, i: float(np.sqrt(np.mean((a[sl, :, i] - truth[sl, :, i]) ** 2)))
    return rms(x_est, 1) / rms(x_proj, 1), rms(x_est, 2) / rms(x_proj, 2)
