"""Raw calls and the list of refusals shared by tests/test_nmpc_loop_cpu.py and tests/test_nmpc_loop_gpu.py: the two
cl_nmpc entries and fsaempc_sqp_batch_device_m.  Every refusal is decided before any launch, so the same list runs on host buffers
without a device."""
import ctypes as C

import numpy as np

DT = 0.05
SENTINEL = -777.0


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def shift_entry(L, N, batch, shift, u_keep, finished, u_init, skip):
    return L.fsaempc_cl_nmpc_shift_batch_device(N, batch, shift, _p(u_keep), _p(finished), _p(u_init), _p(skip), None)


def accept_entry(L, model, N, batch, x_new, u_new, status, qp_iter, skip, x_keep, u_keep, exitflag, it):
    return L.fsaempc_cl_nmpc_accept_batch_device(model, N, batch, _p(x_new), _p(u_new), _p(status), _p(qp_iter), _p(skip), _p(x_keep), _p(u_keep),
                                                 _p(exitflag), _p(it), None)


def check_abi_refusals(device):
    """Every FSAEMPC_ERR_ARG case of fsaempc_cl_nmpc_shift_batch_device, fsaempc_cl_nmpc_accept_batch_device and
    fsaempc_sqp_batch_device_m returns that code with its text and leaves the output buffers untouched; batch 0 succeeds without a
    launch."""
    import torch
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    err = lambda: L.fsaempc_last_error()
    nb, hor = 3, 4
    f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=device)
    i32 = lambda *s: torch.full(s, 7, dtype=torch.int32, device=device)

    # ---- shift ----
    b = dict(u_keep=f64(nb, hor, 2), finished=i32(nb), u_init=f64(nb, hor, 2), skip=i32(nb))

    def sh(N=hor, batch=nb, shift=1, null=(), **repl):
        t = {k: (None if k in null else repl.get(k, b[k])) for k in b}
        return shift_entry(L, N, batch, shift, t["u_keep"], t["finished"], t["u_init"], t["skip"])
    for k in ("u_keep", "u_init", "skip"):
        assert sh(null=(k,)) == -1 and b"null" in err(), k
    for kw in (dict(N=0), dict(N=-3), dict(batch=-1)):
        assert sh(**kw) == -1 and b"dimensions" in err(), kw
    for s in (-1, 2):
        assert sh(shift=s) == -1 and b"shift" in err(), s
    assert sh(u_init=b["u_keep"]) == -1 and b"alias" in err()                                  # the same buffer
    whole = f64(2 * nb * hor * 2)
    assert sh(u_keep=whole[: nb * hor * 2], u_init=whole[2:2 + nb * hor * 2]) == -1 and b"alias" in err()   # overlapping by all but one pair
    assert sh(batch=0) == 0 and sh(batch=0, null=("finished",)) == 0
    assert all(bool((t == 7).all()) for t in b.values())

    # ---- accept ----
    for model, nx in ((0, 5), (1, 7)):
        a = dict(x_new=f64(nb, hor * nx), u_new=f64(nb, hor * 2), status=i32(nb), qp_iter=i32(nb), skip=i32(nb), x_keep=f64(nb, hor, nx),
                 u_keep=f64(nb, hor, 2), exitflag=i32(nb), it=i32(nb))

        def ac(model_=model, N=hor, batch=nb, null=()):
            t = {k: (None if k in null else a[k]) for k in a}
            return accept_entry(L, model_, N, batch, *[t[k] for k in ("x_new", "u_new", "status", "qp_iter", "skip", "x_keep", "u_keep", "exitflag", "it")])
        for k in ("x_new", "u_new", "status", "x_keep", "u_keep", "exitflag", "it"):
            assert ac(null=(k,)) == -1 and b"null" in err(), k
        for m in (2, -1):
            assert ac(model_=m) == -1 and b"model" in err(), m
        for kw in (dict(N=0), dict(batch=-1)):
            assert ac(**kw) == -1 and b"dimensions" in err(), kw
        assert ac(batch=0) == 0 and ac(batch=0, null=("qp_iter", "skip")) == 0
        assert all(bool((t == 7).all()) for t in a.values())

    # ---- the SQP with a skip mask ----
    for model, nx, ns in ((0, 5, 1), (1, 7, 4)):
        table = torch.zeros(8 * 4, dtype=torch.float64, device=device)     # (a spline table is only pointed at: nothing is launched)
        sp = _lib.Spline(4, 1.0, _p(table), _p(table))
        q = dict(x0=f64(nb, nx), x_ref=f64(nb, hor * nx), u_init=f64(nb, hor * 2), skip=i32(nb), u_opt=f64(nb, hor * 2), x_opt=f64(nb, hor * nx),
                 slack=f64(nb, ns), fval=f64(nb), status=i32(nb), sweeps=i32(nb), ws=f64(16))

        def sq(model_=model, N=hor, batch=nb, dt=DT, integ=-1, null=(), desc=True, spl=True, ws_bytes=10 ** 12, **opt):
            d = _lib.LtvDesc(model_, N, batch, dt, integ)
            o = _lib.sqp_default_opts(**opt)
            t = {k: (None if k in null else q[k]) for k in q}
            return L.fsaempc_sqp_batch_device_m(C.byref(d) if desc else None, C.byref(sp) if spl else None, None, _p(t["x0"]), _p(t["x_ref"]),
                                                _p(t["u_init"]), _p(t["skip"]), None, C.byref(o), _p(t["u_opt"]), _p(t["x_opt"]), _p(t["slack"]),
                                                _p(t["fval"]), _p(t["status"]), _p(t["sweeps"]), None, _p(t["ws"]), ws_bytes, None)
        for k in ("x0", "x_ref", "u_init", "u_opt", "x_opt", "slack", "fval", "status", "sweeps", "ws"):
            assert sq(null=(k,)) == -1 and b"null" in err(), k
        for kw in (dict(desc=False), dict(spl=False)):
            assert sq(**kw) == -1 and b"null" in err(), kw
        assert sq(model_=2) == -1 and b"model" in err()
        for kw in (dict(N=0), dict(batch=-1), dict(dt=0.0), dict(integ=3)):
            assert sq(**kw) == -1 and len(err()) > 0, kw
        for kw in (dict(max_sweeps=0), dict(trials=0), dict(trials=65), dict(tol_step=-1.0), dict(tol_feas=float("nan")), dict(armijo=-1.0), dict(rho0=-1.0)):
            assert sq(**kw) == -1 and b"SQP options" in err(), kw
        assert sq(ws_bytes=8) == -5 and b"workspace" in err()               # FSAEMPC_ERR_WORKSPACE: the 16-double buffer is never written
        assert sq(batch=0) == 0 and sq(batch=0, null=("skip",)) == 0
        assert all(bool((t == 7).all()) for t in q.values())
