"""CPU tests of the parameter blocks (fsaempc_ltv_params): the numpy statement of the models with a block as
argument (tests/param_numpy.py) is pinned to the oracle and to tests/nlp_numpy.py at the defaults; the header, the library and the
Python mirror agree on the block; the device entries compute nothing without a GPU; param_draws is a pure function of the id."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nlp_numpy as nn
import param_numpy as pn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["fsaempc_ltv_default_params", "fsaempc_ltv_build_qp_batch_device_p", "fsaempc_ltv_step_batch_device_p",
       "fsaempc_nlp_build_qp_batch_device_p", "fsaempc_sqp_batch_device_p", "fsaempc_cl_plant_batch_device_p"]
TABLE = dict(M=280, IZ=200, LF=0.8672, LR=0.6183, GRAV=9.81, PB=12.56, PC=1.38, PD=1.60, PE=-0.58, Q_S=5, Q_N=250, Q_MU=2000,
             Q_TERMINAL=10, R_ACC=10, R_STEER=10, R_SOFT0=1e8, R_SOFT1=1e6, R_SOFT2=1e6, R_SOFT3=1e4, U_ACC_MAX=10, U_STEER_MAX=0.4,
             DELTA_MAX=0.4, N_MAX=0.75, V_MIN=0, ALAT_MAX=5, SLIP_MAX=0.1, ELL_LONG=10.0, ELL_LAT=9.163, PID_KP_V=16000,
             PID_MAX_F=2800, PID_KP_D=80, PID_MAX_DRATE=0.8)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _rand_state(model, rng, L):
    x = [rng.uniform(0, L), rng.uniform(-0.5, 0.5), rng.uniform(-0.1, 0.1), rng.uniform(5, 20)]
    x += [rng.uniform(-0.1, 0.1)] if model == 0 else [rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)]
    return np.array(x)


@pytest.mark.parametrize("model", [0, 1])
def test_numpy_models_equal_the_oracle_at_the_default_block(orc, otrack, model):
    import fsae_mpc_amd as fm
    P = fm.default_params(model)
    rng = np.random.default_rng(100 + model)
    N = 8
    for _ in range(64):
        x = _rand_state(model, rng, otrack.L)
        u = np.array([rng.uniform(-10, 10), rng.uniform(-0.4, 0.4)])
        assert _rel(pn.f_model(P, orc, model, otrack, x, u), orc.f_model(model, otrack, x, u)) <= 1e-12
        c = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3), rng.uniform(1, 20), rng.uniform(-0.5, 0.5),
                      rng.uniform(-0.5, 0.5), rng.uniform(-0.3, 0.3)])
        uc = np.array([rng.uniform(-2800, 2800), rng.uniform(-0.8, 0.8)])
        assert _rel(pn.f_cart_dyn(P, c, uc), orc.f_cart_dyn(c, uc)) <= 1e-12
        pid = rng.uniform(-1, 1, 4)
        v_ref, d_ref = rng.uniform(0, 20), rng.uniform(-0.3, 0.3)
        for a, b in zip(pn.plant_step(P, c, pid, v_ref, d_ref, 0.05), orc.plant_step(c, pid, v_ref, d_ref, 0.05)):
            assert _rel(a, b) <= 1e-12
        # the NLP pieces on a short random trajectory
        X = np.array([_rand_state(model, rng, otrack.L) for _ in range(N)])
        U = np.stack([rng.uniform(-10, 10, N), rng.uniform(-0.4, 0.4, N)], 1)
        xr = X + rng.uniform(-1, 1, X.shape)
        s = rng.uniform(0, 0.1, 1 if model == 0 else 4)
        assert _rel(pn.rows(P, model, X, U), nn.rows(model, X, U)) <= 1e-12
        assert _rel(pn.slack_min(P, model, X, U), nn.slack_min(model, X, U)) <= 1e-12
        assert _rel(pn.objective(P, model, X, U, s, xr), nn.objective(model, X, U, s, xr)) <= 1e-12
        assert _rel(pn.hard_violation(P, X), nn.hard_violation(X)) <= 1e-12
    # and one rollout through the integrators
    x0 = _rand_state(model, rng, otrack.L)
    U = np.stack([rng.uniform(-2, 2, N), rng.uniform(-0.05, 0.05, N)], 1)
    for integ in (0, 1, 2):
        assert _rel(pn.rollout(P, orc, model, otrack, x0, U, 0.05, integ), nn.rollout(orc, model, otrack, x0, U, 0.05, integ)) <= 1e-12


def test_default_params_index_and_struct_match_the_header(tmp_path):
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define FSAEMPC_P_([A-Z_0-9]+)\s+(\d+)", hdr)}
    assert int(re.search(r"#define FSAEMPC_NPAR\s+(\d+)", hdr).group(1)) == 32 == fm.NPAR == len(macros)
    assert macros == fm.PARAM_INDEX == pn.IDX and sorted(macros.values()) == list(range(32))
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        P = fm.default_params(model)
        assert P.shape == (32,) and P.dtype == np.float64
        for name, v in TABLE.items():
            if model == fm.KINEMATIC and name in ("R_SOFT1", "R_SOFT2", "R_SOFT3"):
                assert P[macros[name]] == 0.0, name        # the kinematic model has the one slack of entry 15
            else:
                assert P[macros[name]] == float(v), name
    assert fm.lib().fsaempc_ltv_default_params(7, fm.default_params(0).ctypes.data_as(C.POINTER(C.c_double))) < 0
    assert fm.lib().fsaempc_ltv_default_params(0, None) < 0
    # the struct, as the C compiler lays it out (the method of test_struct_layouts_of_the_python_mirror_match_the_header)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsaempc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(fsaempc_ltv_params), offsetof(fsaempc_ltv_params, values), '
                   'offsetof(fsaempc_ltv_params, per_instance));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = _lib.LtvParams
    assert out == [C.sizeof(S), S.values.offset, S.per_instance.offset], out


def test_parameterised_entries_are_exported_and_compute_nothing_without_a_gpu():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s), s
    if torch.cuda.is_available():
        return     # the rest states what happens without a device
    tr = fm.Track.load("fsg2019")
    N, B = 10, 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        x0, xl, ul, xr = fm.instances(model, N, 0.05, tr.L, 31, range(B))
        P = fm.default_params(model)
        sb = fm.SqpBatch(model, N, 0.05, tr, B, device="cpu", params=P)
        with pytest.raises(fm.FsaempcError):
            sb.solve(t(x0), t(xr), t(ul))
        with pytest.raises(fm.FsaempcError):
            sb.build_qp(t(x0), t(xr), t(ul))
        # the raw entries: an error code and untouched outputs
        nx, ns, nV, nC = fm.dims(model, N)
        desc = fm._lib.LtvDesc(model, N, B, 0.05, -1)
        xP, yP = t(tr.xP.T), t(tr.yP.T)
        sp = fm._lib.Spline(tr.M, tr.dl, C.c_void_p(xP.data_ptr()), C.c_void_p(yP.data_ptr()))
        par = t(np.stack([P, P]))
        pc = fm._lib.LtvParams(C.c_void_p(par.data_ptr()), 1)
        p = lambda a: C.c_void_p(a.data_ptr())
        outs = [torch.full((B * n,), 7.0, dtype=torch.float64) for n in (nV * nV, nV, nC * nV, nV, nV, nC, nC, nx * N, nx * N * nV, 1)]
        rc = L.fsaempc_ltv_build_qp_batch_device_p(C.byref(desc), C.byref(sp), C.byref(pc), p(t(x0)), p(t(xr)), p(t(xl)), p(t(ul)),
                                                   *[p(o) for o in outs], None)
        assert rc < 0 and all(bool((o == 7.0).all()) for o in outs)
        rc = L.fsaempc_nlp_build_qp_batch_device_p(C.byref(desc), C.byref(sp), C.byref(pc), p(t(x0)), p(t(xr)), p(t(ul)),
                                                   *[p(o) for o in outs], None)
        assert rc < 0 and all(bool((o == 7.0).all()) for o in outs)
        ws = torch.zeros(max(1, L.fsaempc_ltv_workspace_bytes(C.byref(desc)) // 8 + 1), dtype=torch.float64)
        res = [torch.full((B * n,), 7.0, dtype=torch.float64) for n in (2 * N, nx * N, ns, 1)]
        fl, it = torch.full((B,), 7, dtype=torch.int32), torch.full((B,), 7, dtype=torch.int32)
        rc = L.fsaempc_ltv_step_batch_device_p(C.byref(desc), C.byref(sp), C.byref(pc), p(t(x0)), p(t(xr)), p(t(xl)), p(t(ul)), None,
                                               *[p(o) for o in res], p(fl), p(it), None, None, p(ws), C.c_longlong(ws.numel() * 8), None)
        assert rc < 0 and all(bool((o == 7.0).all()) for o in res) and bool((fl == 7).all())
        cart, pid = torch.full((B, 7), 7.0, dtype=torch.float64), torch.zeros((B, 4), dtype=torch.float64)
        rc = L.fsaempc_cl_plant_batch_device_p(model, N, C.c_double(0.05), B, C.byref(pc), p(cart), p(pid), p(res[1]), None, None, None, None)
        assert rc < 0 and bool((cart == 7.0).all())


def test_param_draws_are_a_pure_function_of_the_id():
    import fsae_mpc_amd as fm
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        alone = fm.param_draws(model, np.arange(100, 164), 20190, 0.1)
        inside = fm.param_draws(model, np.arange(4096), 20190, 0.1)
        assert alone.shape == (64, 32) and np.array_equal(alone, inside[100:164])
        d = fm.default_params(model)
        rel = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14, 19, 20, 21, 22, 23, 24, 25, 26, 27]
        fixed = [4, 8, 28, 29, 30, 31]
        assert np.array_equal(inside[:, fixed], np.repeat(d[None, fixed], 4096, 0))
        assert np.all(np.abs(inside[:, rel] - d[rel]) <= 0.1 * np.abs(d[rel]) * (1 + 1e-15))
        nz = [j for j in rel if d[j] != 0]
        assert np.all(np.ptp(inside[:, nz], axis=0) > 0.15 * np.abs(d[nz]))           # the draws fill the range
        soft = [15] if model == fm.KINEMATIC else [15, 16, 17, 18]
        r = inside[:, soft] / d[soft]
        assert np.all((r >= 0.1 * (1 - 1e-12)) & (r <= 10 * (1 + 1e-12))) and np.all(r.max(0) > 5) and np.all(r.min(0) < 0.2)
        assert not np.array_equal(fm.param_draws(model, np.arange(8), 1, 0.1), inside[:8])   # the seed matters
        assert np.array_equal(fm.param_draws(model, np.arange(8), 20190, 0.0)[:, rel], np.repeat(d[None, rel], 8, 0))
