"""Inputs and raw calls shared by tests/test_estimator_cpu.py and tests/test_estimator_gpu.py: a direct ctypes call of
fsaempc_cl_estimate_batch_device on numpy inputs and the list of its refusals (decided before any launch, so the same list runs on
host buffers without a device)."""
import ctypes as C

import numpy as np

DT = 0.05
B, N = 70, 10      # nine wavefronts of 8 cars, the last group of lanes partial


def estimate(fm, torch, tr, model, *, z, x_start, u_prev, q, r, p0, L=0.0, finished=None, est_x=None, est_P=None, est_count=None, params=None,
             integrator=-1, horizon=N, want=True, device="cuda"):
    """fsaempc_cl_estimate_batch_device on numpy inputs.  u_prev: (batch, horizon, 2) plans (stage 1 is read) or (batch, 2).  Returns a dict of
    numpy arrays: est_x, est_P, est_count, x0_est, innov, nis and (want) F_out, x_prior."""
    from fsae_mpc_amd import _lib
    batch, nx = z.shape
    dev = lambda a, dt=torch.float64: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt, device=device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    mpc = fm.LtvBatch(model, horizon, DT, tr, batch, integrator=integrator, params=params, device=device)
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    tq, tr_, tp0, tz, txs, tu, tfin = dev(q), dev(r), dev(p0), dev(z), dev(x_start), dev(u_prev), dev(finished, torch.int32)
    est = _lib.ClEstimator(p(tq), 1 if q.ndim == 2 else 0, p(tr_), 1 if r.ndim == 2 else 0, p(tp0), float(L))
    ex = dev(est_x) if est_x is not None else torch.full((batch, nx), 123.0, dtype=torch.float64, device=device)
    eP = dev(est_P) if est_P is not None else torch.full((batch, nx, nx), 123.0, dtype=torch.float64, device=device)
    ec = dev(est_count, torch.int32) if est_count is not None else torch.zeros((batch, 2), dtype=torch.int32, device=device)
    f64 = lambda *s: torch.full(s, -777.0, dtype=torch.float64, device=device)
    x0e, inn, nis = f64(batch, nx), f64(batch, nx), f64(batch)
    Fo, xp = (f64(batch, nx, nx), f64(batch, nx)) if want else (None, None)
    rc = fm.lib().fsaempc_cl_estimate_batch_device(C.byref(mpc.desc), C.byref(mpc.sp), mpc.params.ref() if mpc.params is not None else None, C.byref(est),
                                                   p(tz), p(txs), p(tu), int(np.prod(u_prev.shape[1:])), p(tfin), p(ex), p(eP), p(ec), p(x0e), p(inn), p(nis),
                                                   p(Fo), p(xp), None)
    _lib.check(rc, "fsaempc_cl_estimate_batch_device")
    torch.cuda.synchronize()
    g = lambda t: None if t is None else t.cpu().numpy()
    return dict(est_x=g(ex), est_P=g(eP), est_count=g(ec), x0_est=g(x0e), innov=g(inn), nis=g(nis), F_out=g(Fo), x_prior=g(xp))


def check_abi_refusals(device):
    """Every FSAEMPC_ERR_ARG case of fsaempc_cl_estimate_batch_device returns that code with its text and leaves the buffers untouched;
    batch 0 succeeds without a launch."""
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
        names = ("z", "x_start", "u_prev", "finished", "est_x", "est_P", "est_count", "x0_est", "innov", "nis", "F_out", "x_prior")
        big = f64(nb * nx * nx + nb * nx)                                  # (one allocation two outputs can share)
        bufs = dict(z=f64(nb, nx), x_start=f64(nb, nx), u_prev=f64(nb, hor, 2), finished=torch.zeros(nb, dtype=torch.int32, device=device),
                    est_x=f64(nb, nx), est_P=f64(nb, nx, nx), est_count=torch.full((nb, 2), 7, dtype=torch.int32, device=device), x0_est=f64(nb, nx),
                    innov=f64(nb, nx), nis=f64(nb), F_out=f64(nb, nx, nx), x_prior=f64(nb, nx))
        var = dict(q=f64(nx), r=f64(nx), p0=f64(nx))

        def call(model_=model, N_=hor, batch=nb, dt=DT, integ=-1, Lap=0.0, stride=2 * hor, null=(), swap=None, desc=True, spl=True, est=True):
            d = _lib.LtvDesc(model_, N_, batch, dt, integ)
            v = {k: (None if k in null else p(var[k])) for k in var}
            e = _lib.ClEstimator(v["q"], 0, v["r"], 0, v["p0"], Lap)
            ptr = {k: (None if k in null else p(bufs[k])) for k in names}
            ptr.update(swap or {})
            a = [ptr[k] for k in names]
            return L.fsaempc_cl_estimate_batch_device(C.byref(d) if desc else None, C.byref(sp) if spl else None, None, C.byref(e) if est else None,
                                                      a[0], a[1], a[2], stride, *a[3:], None)
        assert call(batch=0) == 0 and call(batch=0, null=("finished", "F_out", "x_prior")) == 0      # nothing to launch
        for kw in (dict(desc=False), dict(spl=False), dict(est=False)):
            assert call(**kw) == -1 and b"null" in err(), kw
        for k in ("q", "r", "p0", "z", "x_start", "u_prev", "est_x", "est_P", "est_count", "x0_est", "innov", "nis"):
            assert call(null=(k,)) == -1 and b"null" in err(), k
        assert call(model_=2) == -1 and b"model" in err()
        for kw in (dict(N_=0), dict(batch=-1), dict(dt=0.0), dict(integ=3), dict(integ=-2)):
            assert call(**kw) == -1 and len(err()) > 0, kw
        for Lap in (-1.0, float("inf"), float("nan")):
            assert call(Lap=Lap) == -1 and b"L must" in err(), Lap
        for stride in (1, 0, -4):
            assert call(stride=stride) == -1 and b"u_stride" in err(), stride
        # overlapping outputs: the same buffer twice, a partial overlap inside one allocation, an output on top of an input
        assert call(swap=dict(x0_est=p(bufs["est_x"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(innov=p(bufs["x_prior"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(est_P=C.c_void_p(big.data_ptr()), est_x=C.c_void_p(big.data_ptr() + 8 * (nb * nx * nx - 1)))) == -1 and b"overlap" in err()
        assert call(swap=dict(x0_est=p(bufs["z"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(est_x=p(bufs["x_start"]))) == -1 and b"overlap" in err()
        assert call(swap=dict(nis=p(var["p0"]))) == -1 and b"overlap" in err()
        assert all(bool((bufs[k] == 7).all()) for k in names if k != "finished") and bool((big == 7).all())
