"""Inputs and raw calls shared by tests/test_latency_cpu.py and tests/test_latency_gpu.py: the states of the
observation and prediction tests, a direct ctypes call of fsaempc_cl_observe_batch_device, and the list of refusals of the two device
entries (decided before any launch, so the same list runs on host buffers without a device)."""
import ctypes as C
import glob
import os

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT = 0.05
B, N = 70, 10      # more than one wavefront, not a multiple of 64
SEED = 2 ** 40 + 3


def states(model, batch=B):
    """(batch, nx) states: the x0 rows of the fsg2019 golden fixtures of the model, repeated, with speeds spread over 2 .. 15 m/s."""
    rows = []
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "fsg2019_%s_N*.npz" % ("kin" if model == 0 else "dyn")))):
        with np.load(f) as z:
            rows.append(z["x0"])
    rows = np.concatenate(rows)
    x = rows[np.arange(batch) % rows.shape[0]].copy()
    x[:, 0] += 0.37 * np.arange(batch)                  # (not the same track position twice)
    x[:, 3] = np.linspace(2.0, 15.0, batch)
    return x


def input_history(delay, batch=B, horizon=N, seed=5):
    """u_hist (delay + 1, batch, horizon, 2) inside the input box (|a| <= 10, |delta rate| <= 0.4)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.0, 1.0, (delay + 1, batch, horizon, 2))
    u[..., 0] *= 10.0
    u[..., 1] *= 0.4
    return u


def observe(fm, torch, tr, model, x0, *, delay=0, compensate=0, sigma=None, seed=SEED, id0=0, step=0, finished=None, u_hist=None, params=None,
            integrator=-1, horizon=N, device="cuda"):
    """fsaempc_cl_observe_batch_device on numpy inputs; returns (x0_obs, x0_mpc) as numpy."""
    from fsae_mpc_amd import _lib
    batch, nx = x0.shape
    dev = lambda a, dt=torch.float64: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt, device=device)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    mpc = fm.LtvBatch(model, horizon, DT, tr, batch, integrator=integrator, params=params, device=device)
    sg, fin, uh, xt = dev(sigma), dev(finished, torch.int32), dev(u_hist), dev(x0)
    lat = _lib.ClLatency(delay, compensate, p(sg), 1 if sg is not None and sg.dim() == 2 else 0, seed, id0)
    obs = torch.full((batch, nx), -777.0, dtype=torch.float64, device=device)
    mp = torch.full((batch, nx), -777.0, dtype=torch.float64, device=device)
    rc = fm.lib().fsaempc_cl_observe_batch_device(C.byref(mpc.desc), C.byref(mpc.sp), mpc.params.ref() if mpc.params is not None else None, C.byref(lat),
                                                  step, p(xt), p(fin), p(uh), p(obs), p(mp), None)
    _lib.check(rc, "fsaempc_cl_observe_batch_device")
    torch.cuda.synchronize()
    return obs.cpu().numpy(), mp.cpu().numpy()


def check_abi_refusals(device):
    """Every FSAEMPC_ERR_ARG case of fsaempc_cl_noise_batch_device and fsaempc_cl_observe_batch_device returns that code with its text
    and leaves the output buffers untouched; batch 0 succeeds without a launch."""
    import torch
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    err = lambda: L.fsaempc_last_error()
    nb, hor = 3, 4
    for nx in (5, 7):
        z = torch.full((nb, nx), 7.0, dtype=torch.float64, device=device)
        noise = lambda nx_=nx, batch=nb, seed=1, id0=0, step=0, out=z: L.fsaempc_cl_noise_batch_device(nx_, batch, seed, id0, step, p(out), None)
        for kw in (dict(nx_=6), dict(nx_=0), dict(nx_=8)):
            assert noise(**kw) == -1 and b"nx" in err(), kw
        assert noise(batch=-1) == -1 and len(err()) > 0
        assert noise(id0=-1) == -1 and b"id0" in err()
        for step in (-1, 2 ** 32, 2 ** 40):
            assert noise(step=step) == -1 and b"step" in err(), step
        assert noise(out=None) == -1 and b"null" in err()
        assert noise(batch=0) == 0
        assert bool((z == 7).all())

        model = 0 if nx == 5 else 1
        table = torch.zeros(8 * 4, dtype=torch.float64, device=device)     # (a spline table is only pointed at: nothing is launched)
        sp = _lib.Spline(4, 1.0, p(table), p(table))
        f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=device)
        bufs = dict(x0_true=f64(nb, nx), finished=torch.zeros(nb, dtype=torch.int32, device=device), u_hist=f64(3, nb, hor, 2), x0_obs=f64(nb, nx),
                    x0_mpc=f64(nb, nx))
        sigma = f64(nx)

        def obs(model_=model, N_=hor, batch=nb, dt=DT, integ=-1, delay=2, comp=1, id0=0, step=0, null=(), desc=True, spl=True, lat=True):
            d = _lib.LtvDesc(model_, N_, batch, dt, integ)
            la = _lib.ClLatency(delay, comp, p(sigma), 0, 1, id0)
            return L.fsaempc_cl_observe_batch_device(C.byref(d) if desc else None, C.byref(sp) if spl else None, None, C.byref(la) if lat else None, step,
                                                     *[None if k in null else p(bufs[k]) for k in ("x0_true", "finished", "u_hist", "x0_obs", "x0_mpc")], None)
        for kw in (dict(delay=-1), dict(delay=5)):
            assert obs(**kw) == -1 and b"delay" in err(), kw
        assert obs(comp=2) == -1 and b"compensate" in err()
        for step in (-1, 2 ** 32):
            assert obs(step=step) == -1 and b"step" in err(), step
        assert obs(id0=-1) == -1 and b"id0" in err()
        assert obs(model_=2) == -1 and b"model" in err()                   # (nx not 5 or 7: the model of the descriptor)
        assert obs(null=("u_hist",)) == -1 and b"u_hist" in err()
        assert obs(null=("u_hist",), delay=1, comp=0) == -1 and b"u_hist" in err()
        for k in ("x0_true", "x0_obs", "x0_mpc"):
            assert obs(null=(k,)) == -1 and b"null" in err(), k
        for kw in (dict(desc=False), dict(spl=False), dict(lat=False)):
            assert obs(**kw) == -1 and b"null" in err(), kw
        for kw in (dict(N_=0), dict(batch=-1), dict(dt=0.0), dict(integ=3), dict(integ=-2)):
            assert obs(**kw) == -1 and len(err()) > 0, kw
        assert obs(batch=0) == 0 and obs(batch=0, delay=0, comp=0, null=("u_hist", "finished")) == 0   # nothing to launch
        assert all(bool((bufs[k] == 7).all()) for k in ("x0_true", "u_hist", "x0_obs", "x0_mpc"))
