"""The reference side of tests/test_qp_shapes_gpu.py, on the CPU alone: the oracle meets every condition the GPU tests impose on
the generic QP families (tests/qp_families.py) and on the LTV-MPC QPs with 2- and 3-column borders, and its active-set refinement
returns nothing that is not a KKT point (it accepted candidates on feasibility and multiplier signs alone: flag 0, polished = 1,
certificate 4.3e-5 on dynamic N = 80, 4e-2 on a QP of family R)."""
import numpy as np
import pytest

import qp_families as qf
from kkt_numpy import kkt_certificate

KKT_TOL = 1e-6          # tests/test_gpu_parity.py
FVAL_TOL = 1e-6
X_STAR_TOL = 1e-9       # closed-form minimisers (families F, E)
POLISH_ACCEPT = 1e-8    # oracle/ltv_oracle_qp.c: a refined point is returned only with a certificate at this level
B = 8

LTV_BORDER_SHAPES = [(1, 7, 24), (1, 23, 24), (1, 39, 24), (1, 55, 24), (1, 63, 12),      # dynamic: nV = 2N + 4 = 2 (mod 16)
                     (0, 9, 24), (0, 25, 24), (0, 41, 24), (0, 57, 24), (0, 65, 12)]      # kinematic: nV = 2N + 1 = 3 (mod 16)
LTV_SEED = 404


def _args(q):
    return [q[k] for k in qf.KEYS]


def _orc_kkt(orc, q, sol):
    return np.array([orc.qp_kkt(q["H"][b].T, q["g"][b], q["A"][b].T, q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b], sol["x"][b], sol["lam"][b])[0]
                     for b in range(len(q["g"]))])


def test_families_are_deterministic_and_as_described():
    a, b = qf.make("R", 35, 50, 3), qf.make("R", 35, 50, 3)
    assert all(np.array_equal(a[k], b[k]) for k in qf.KEYS)
    assert not np.array_equal(a["g"], qf.make("R", 35, 50, 4)["g"])
    A = a["A"]
    assert not A[1].any() and (a["lbA"][1], a["ubA"][1]) == (-1.0, 1.0)
    assert np.nonzero(A[2])[0].tolist() == [34]
    assert np.array_equal(A[3], A[4]) and a["lbA"][3] == a["lbA"][4] and a["ubA"][3] == a["ubA"][4]
    assert a["lb"][3] == a["ub"][3]
    last = np.array([np.nonzero(r)[0].max() for r in A[5:]])
    assert (np.diff(last) < 0).any() and (np.diff(last) > 0).any()            # the staircase is not sorted
    mx = np.abs(A[5:]).max(axis=1)
    assert mx.max() / mx.min() > 1e4                                          # row scales over decades
    assert np.linalg.eigvalsh(a["H"]).min() > 0.99 and np.array_equal(a["H"], a["H"].T)
    s = qf.make("S", 35, 50, 0)
    assert not s["H"][-1].any() and not s["H"][:, -1].any() and s["g"][-1] == 1e6 and (s["lb"][-1], s["ub"][-1]) == (0.0, np.inf)
    assert np.isinf(s["lbA"]).all() and np.array_equal(s["A"][:, -1], np.where(np.arange(50) % 3 == 0, -1.0, 0.0))
    sh = [qf.make("R", 52, 70, i, ha_inst=0) for i in range(3)]
    assert np.array_equal(sh[0]["A"], sh[2]["A"]) and not np.array_equal(sh[0]["lbA"], sh[2]["lbA"])
    f = qf.make("F", 20, 0, 0)
    assert f["A"].shape == (0, 20) and (np.abs(np.concatenate([f["lb"], f["ub"]])) >= 1e9).all()
    bad = qf.make_infeasible(52, 70, 0)
    assert bad["lbA"][4] > bad["ubA"][3] and np.array_equal(bad["A"][3], bad["A"][4])


def test_shapes_reach_the_layouts_they_are_meant_for():
    """fsaempc_qp_layout (a host function): (21, 60) and (24, 200) carry the LTV signature and get the dummy-padded core with a 1- /
    4-column border, every other shape of the list is solved in the caller's numbering; the LTV border shapes run the NB = 4
    kernels unpadded; the list reaches both solve kernels, border widths 0, 2, 3 and 4, and a zero-curvature column inside the core."""
    import fsae_mpc_amd as fm
    assert fm.qp_layout(21, 60) == dict(T=2, NB=1, n_solver=33, wavefront_kernel=True)
    assert fm.qp_layout(24, 200) == dict(T=2, NB=4, n_solver=36, wavefront_kernel=True)
    lay = {s: fm.qp_layout(*s) for s in qf.SHAPES[:-2] + qf.SHAPES_F_ONLY}
    assert all(v["n_solver"] == s[0] for s, v in lay.items())
    assert {s[0] % 16 for s, v in lay.items() if v["NB"] == 4} == {2, 3, 4} and {s[0] for s, v in lay.items() if v["NB"] == 0} == {15, 16, 96, 117}
    assert {v["wavefront_kernel"] for v in lay.values()} == {True, False}
    for model, N, _ in LTV_BORDER_SHAPES:
        nV, nC = (2 * N + 4, 20 * N) if model else (2 * N + 1, 6 * N)
        assert fm.qp_layout(nV, nC) == dict(T=nV // 16, NB=4, n_solver=nV, wavefront_kernel=nV <= 116), (model, N)


@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in qf.FAMILIES for n, m in qf.shapes(f)])
def test_oracle_on_generic_families(orc, family, nV, nC):
    """Flag 0, the numpy certificate <= 1e-6, the closed-form minimiser to 1e-9, refinement on and off agree in fval to 1e-6, and no
    refined point without its certificate (no refinement RATE is asserted: dependent active rows of family R end the LU refinement)."""
    q = qf.batch(family, nV, nC, B)
    on = orc.qp_solve_batch_aux(*_args(q))
    off = orc.qp_solve_batch_aux(*_args(q), opts=orc.default_opts(polish=0))
    for tag, sol in (("on", on), ("off", off)):
        assert (sol["exitflag"] == 0).all(), (tag, sol["exitflag"])
        c = kkt_certificate(*_args(q), sol["x"], sol["lam"])
        assert c["max"].max() <= KKT_TOL, (tag, {k: float(np.max(c[k])) for k in ("stationarity", "primal", "sign", "complementarity")})
    assert (off["polished"] == 0).all()
    assert (np.abs(on["fval"] - off["fval"]) <= FVAL_TOL * np.maximum(1.0, np.abs(off["fval"]))).all()
    if "x_star" in q:
        err = np.abs(on["x"] - q["x_star"]).max(axis=1) / np.maximum(1.0, np.abs(q["x_star"]).max(axis=1))
        assert err.max() <= X_STAR_TOL, err
    kk = _orc_kkt(orc, q, on)
    assert not ((on["polished"] > 0) & (kk > POLISH_ACCEPT)).any(), (on["polished"], kk)


@pytest.mark.parametrize("model,N,nb", LTV_BORDER_SHAPES)
def test_oracle_on_ltv_border_2_and_3(orc, otrack, model, N, nb):
    x0, xl, ul, xr = orc.synth_instances(model, N, 0.05, otrack.L, LTV_SEED, range(nb))
    q = orc.build_qp_batch(model, otrack, N, 0.05, x0, xr, xl, ul)
    assert q["g"].shape[1] % 16 == (2 if model == 1 else 3)
    ref = orc.qp_solve_batch_aux(*_args(q))
    assert (ref["exitflag"] == 0).all(), ref["exitflag"]
    assert kkt_certificate(*_args(q), ref["x"], ref["lam"])["max"].max() <= KKT_TOL


@pytest.mark.parametrize("N,nb", [(80, 16), (60, 24)])
def test_refinement_returns_only_kkt_points(orc, otrack, N, nb):
    """Dynamic N = 80 x 16 and N = 60 x 24 of the synthetic family: before the fresh certificate in polish() one instance of each
    came back flag 0, polished = 1 with orc_qp_kkt = 4.3e-5 / 6.2e-7 (the LU solution of its working set was not stationary)."""
    x0, xl, ul, xr = orc.synth_instances(1, N, 0.05, otrack.L, 20190, range(nb))
    q = orc.build_qp_batch(1, otrack, N, 0.05, x0, xr, xl, ul)
    ref = orc.qp_solve_batch_aux(*_args(q))
    assert (ref["exitflag"] == 0).all()
    kk = _orc_kkt(orc, q, ref)
    assert kk.max() <= KKT_TOL
    assert not ((ref["polished"] > 0) & (kk > POLISH_ACCEPT)).any(), (ref["polished"], kk)
    assert (ref["polished"] > 0).sum() >= nb - 2          # the check rejects the bad candidates, not the refinement as a whole
