"""CPU tests of the QP sensitivities: the numpy adjoint (tests/sens_numpy.py) against central differences of the working-set solution
map (kkt_numpy.vertex_from_working_set) on the committed LTV-MPC QPs, and the C declarations of the VJP against the Python bindings."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

import kkt_numpy as kn
import sens_numpy as sn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = sorted(f for f in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")) if not os.path.basename(f).startswith("regress_"))


def _qp(d, b):
    H = d["H"][b].T
    A = d["A"][b].T
    return H, d["g"][b], A, d["lb"][b], d["ub"][b], d["lbA"][b], d["ubA"][b], d["x"][b], d["lam"][b]


@pytest.mark.parametrize("path", GOLDEN[:6], ids=[os.path.basename(p) for p in GOLDEN[:6]])
def test_numpy_adjoint_matches_central_differences_of_the_working_set_map(path):
    d = np.load(path)
    rng = np.random.default_rng(7)
    checked = 0
    for b in range(d["g"].shape[0]):
        H, g, A, lb, ub, lbA, ubA, x, lam = _qp(d, b)
        n, m = len(g), len(lbA)
        ws = sn.working_set_rule(lb, ub, lbA, ubA, x, A, lam)
        x0, _ = kn.vertex_from_working_set(H, g, A, lb, ub, lbA, ubA, ws)
        assert np.max(np.abs(x0 - x)) <= 1e-6 * max(1.0, np.max(np.abs(x)))   # the stored vertex is the one of its working set
        xbar, fbar = rng.standard_normal(n), 0.7
        adj = sn.adjoint(H, g, A, x0, lam, ws, xbar, fbar)
        fval = lambda xx, HH, gg: 0.5 * xx @ HH @ xx + gg @ xx
        dirs = dict(g=rng.standard_normal(n), lb=rng.standard_normal(n), ub=rng.standard_normal(n),
                    lbA=rng.standard_normal(m), ubA=rng.standard_normal(m))
        for key, v in dirs.items():
            # the map is affine in g and the bounds: no truncation error at any h that keeps the working set
            h = 1e-4 * max(1.0, np.max(np.abs({"g": g, "lb": np.where(np.isfinite(lb), lb, 0), "ub": np.where(np.isfinite(ub), ub, 0),
                                                "lbA": np.where(np.abs(lbA) < 1e9, lbA, 0), "ubA": np.where(np.abs(ubA) < 1e9, ubA, 0),
                                                }[key])))
            vals = []
            for s in (1.0, -1.0):
                q = dict(g=g, lb=lb, ub=ub, lbA=lbA, ubA=ubA)
                q[key] = q[key] + s * h * v
                xs, _ = kn.vertex_from_working_set(H, q["g"], A, q["lb"], q["ub"], q["lbA"], q["ubA"], ws)
                vals.append(xbar @ xs + fbar * fval(xs, H, q["g"]))
            fd = (vals[0] - vals[1]) / (2 * h)
            an = float(np.sum(adj[key] * v))
            assert abs(fd - an) <= 1e-6 * max(1.0, abs(an), np.max(np.abs(xbar))), (path, b, key, fd, an)
            checked += 1
    assert checked >= 7


def test_numpy_adjoint_known_answers():
    # 1-D: unconstrained gbar = -xbar / h; an active lower bound passes xbar to lb
    a = sn.adjoint(np.array([[4.0]]), np.array([1.0]), np.zeros((0, 1)), np.array([-0.25]), np.zeros(1), np.array([0]), np.array([2.0]))
    assert np.allclose(a["g"], [-0.5]) and np.allclose(a["lb"], [0.0])
    a = sn.adjoint(np.array([[4.0]]), np.array([1.0]), np.zeros((0, 1)), np.array([0.0]), np.array([1.0]), np.array([-1]), np.array([2.0]))
    assert np.allclose(a["g"], [0.0]) and np.allclose(a["lb"], [2.0])


def test_vjp_declarations_match_the_bindings():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for name in ("fsaempc_qp_vjp_batch_device", "fsaempc_qp_vjp_workspace_bytes", "fsaempc_ltv_affine_maps_batch_device",
                 "fsaempc_ltv_step_batch_device_lambda", "fsaempc_ltv_step_vjp_workspace_bytes", "fsaempc_ltv_step_vjp_batch_device"):
        assert name in fm._lib.EXPORTS
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % name, hdr).group(1)
        nargs = len([a for a in decl.split(",") if a.strip()])
        L = fm.lib()
        assert len(getattr(L, name).argtypes) == nargs, (name, nargs)
    body = re.search(r"typedef struct \{([^{}]*)\} fsaempc_qp_vjp_io;", hdr).group(1)
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f for f, _ in fm._lib.QpVjpIO._fields_]
    assert C.sizeof(fm._lib.QpVjpIO) == 8 * len(fields)
    body = re.search(r"typedef struct \{([^{}]*)\} fsaempc_ltv_vjp_io;", hdr).group(1)
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == [f for f, _ in fm._lib.LtvVjpIO._fields_]
    assert fm.lib().fsaempc_ltv_step_vjp_workspace_bytes(C.byref(fm._lib.LtvDesc(0, 40, 64, 0.05, -1)), 2) > 0
    assert fm.lib().fsaempc_ltv_step_vjp_workspace_bytes(C.byref(fm._lib.LtvDesc(0, 40, 64, 0.05, -1)), 0) == -1
    # sizes / argument checks need no device: bad k, dimensions past the limit, shared_HA with Hbar
    d = fm._lib.QpDesc(81, 240, 4096, 0)
    assert fm.lib().fsaempc_qp_vjp_workspace_bytes(C.byref(d)) > 0
    assert fm.lib().fsaempc_qp_vjp_workspace_bytes(C.byref(fm._lib.QpDesc(200, 10, 1, 0))) == -2
    io = fm._lib.QpVjpIO(1, None, 1, None, None, None, None, 1, None)
    st = np.zeros(1, dtype=np.int32)
    p = C.c_void_p(8)
    rc = fm.lib().fsaempc_qp_vjp_batch_device(C.byref(fm._lib.QpDesc(4, 2, 1, 1)), 1, p, p, p, p, p, p, p, p, p, p, None, None,
                                              C.byref(io), st.ctypes.data_as(C.c_void_p), p, C.c_longlong(1 << 30), None)
    assert rc == -1   # FSAEMPC_ERR_ARG: Hbar with shared H
    rc = fm.lib().fsaempc_qp_vjp_batch_device(C.byref(fm._lib.QpDesc(4, 2, 1, 0)), 0, p, p, p, p, p, p, p, p, p, p, None, None,
                                              C.byref(io), st.ctypes.data_as(C.c_void_p), p, C.c_longlong(1 << 30), None)
    assert rc == -1   # k = 0
