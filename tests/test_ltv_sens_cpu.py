"""The reference side of tests/test_ltv_sens_rows_gpu.py, on the CPU alone: the numpy step VJP (tests/ltv_sens_numpy.py, composed
of the oracle's build, the oracle's solve and sens_numpy.adjoint, its Jacobians of the build from differencing the build) against
central differences of the oracle's own step, and the conditions the inputs of tests/ltv_sens_cases.py are made for, asserted on
the oracle's solve: most of each N = 8 batch is a refined vertex, every row family of the constraint block carries a multiplier on
at least two of them, a slack is non-zero somewhere, and the infeasible instances fail.
Tests that measure print a line starting LTVSENS_CPU before they assert; profiles/sens_shapes/README.md records them."""
import functools
import json
import os

import numpy as np
import pytest

import ltv_sens_cases as lc
import ltv_sens_numpy as ln
import sens_numpy as sn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
H_DIFF = 1e-5
# Directional central differences (h = 1e-5) of the oracle's step against the reference, relative to max(1, |value|), worst over the
# instances whose working set holds at +-h and over the six cotangent sets.  The gap is the differences' own: u_opt, x_opt and slack
# are affine along the direction while the working set holds, so theirs is the rounding of the two solves over 2h, and fval is
# quadratic (truncation h^2 times its curvature) and reaches 1e6.  At h = 1e-6 the same comparison gives 1.3e-7, 1.7e-8, 1.9e-7 and
# 1.6e-7 and at h = 1e-4 below 2e-9 on three cases probed -- the gap falls as h grows, as rounding does -- but every working set of
# kin N = 8 only holds up to 1e-5.  Measured at h = 1e-5: kin N=8 5.0e-9, dyn N=8 1.6e-9, kin N=13 9.8e-9, dyn N=9 1.0e-8; the
# bound is ten times that.
FD_MEASURED = {(0, 8): 5.0e-9, (1, 8): 1.6e-9, (0, 13): 9.8e-9, (1, 9): 1.0e-8}
FD_BOUND = {c: 10.0 * v for c, v in FD_MEASURED.items()}


@functools.lru_cache(maxsize=None)
def _track():
    import oracle
    return oracle.Track.load(os.path.join(ROOT, "fsae-mpc_amd", "tracks", lc.TRACK + ".json"))


def oracle_step(model, N, x0, xr, xl, ul):
    """The oracle's LTV-MPC step on a batch (xr (B, nx N)): its build with pred = A_bar x0 + d_bar, its solve, and the step's
    outputs u_opt, x_opt = pred + Bt z, slack, fval = fval_qp + const."""
    import oracle
    B = len(x0)
    nx = lc.dims(model, N)[0]
    q = oracle.build_qp_batch(model, _track(), N, lc.DT, x0, xr.reshape(B, N, nx), xl, ul, keep_prediction=True)
    q["pred"] = np.einsum("bje,bj->be", q["A_bar"], x0) + q["d_bar"]
    r = oracle.qp_solve_batch_aux(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"])
    out = dict(ubar=r["x"][:, :2 * N], xbar=q["pred"] + np.einsum("bie,bi->be", q["Bt"], r["x"]), sbar=r["x"][:, 2 * N:],
               fbar=r["fval"] + q["const"])
    return q, r, out


@functools.lru_cache(maxsize=None)
def oracle_case(model, N):
    """The case's inputs, the oracle's build and solve on them, the Jacobians of the oracle's build, and the step's outputs at
    +-h along lc.directions with the instances whose working set holds there.  Callers leave it unchanged."""
    import oracle
    oracle.lib()
    d = lc.inputs(model, N)
    B = len(d["x0"])
    nx = lc.dims(model, N)[0]
    x0, xr, xl, ul = d["x0"], d["x_ref"].reshape(B, -1), d["x_lin"], d["u_lin"]
    q, r, out = oracle_step(model, N, x0, xr, xl, ul)

    def build(x0_, xr_):
        qq = oracle.build_qp_batch(model, _track(), N, lc.DT, x0_, xr_.reshape(B, N, nx), xl, ul, keep_prediction=True)
        qq["pred"] = np.einsum("bje,bj->be", qq["A_bar"], x0_) + qq["d_bar"]
        return qq

    jac = ln.build_jacobians(build, x0, xr)
    refined = (r["exitflag"] == 0) & (r["polished"] > 0)
    v0, vr = lc.directions(model, N, B, x0, xr)
    same, side = refined.copy(), []
    for s in (1.0, -1.0):
        _, r1, o1 = oracle_step(model, N, x0 + s * H_DIFF * v0, xr + s * H_DIFF * vr, xl, ul)
        same &= (np.sign(r1["lam"]) == np.sign(r["lam"])).all(axis=1) & (r1["polished"] > 0) & (r1["exitflag"] == 0)
        side.append(o1)
    return dict(inputs=d, q=q, r=r, jac=jac, refined=refined, same=same, v0=v0, vr=vr, plus=side[0], minus=side[1])


def test_key_tolerances_restate_the_tolerance_of_compare():
    """sens_numpy.compare returns error / tolerance only: an output that is off by exactly key_tolerances' figure in its largest
    entry must come back as 1, for each of the three keys, on instances with and without working rows and with fbar."""
    c = oracle_case(0, 8)
    q, r = c["q"], c["r"]
    cot = lc.cotangents(0, 8, len(r["x"]), "all")
    for b in np.nonzero(c["refined"])[0][::5]:
        Hb, Ab = q["H"][b].T, q["A"][b].T
        ws = sn.working_set_rule(q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b], r["x"][b], Ab, r["lam"][b])
        zbar = np.concatenate([cot["ubar"][b, 0], cot["sbar"][b, 0]]) + q["Bt"][b] @ cot["xbar"][b, 0]
        for fbar in (0.0, cot["fbar"][b, 0]):
            ad = sn.adjoint(Hb, q["g"][b], Ab, r["x"][b], r["lam"][b], ws, zbar, fbar)
            kt = ln.key_tolerances(ad, Hb, q["g"][b], Ab, r["x"][b], zbar, fbar)
            for key, t in kt.items():
                got = ad[key].copy()
                got[0] += t
                e, _ = sn.compare({key: got}, ad, Hb, q["g"][b], Ab, r["x"][b], r["lam"][b], zbar, fbar)
                assert abs(e - 1.0) <= 1e-6, (b, key, e)    # ad[key][0] + t - ad[key][0] rounds


@pytest.mark.parametrize("name", lc.COTANGENT_SETS)
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_reference_matches_differences_of_the_oracle_step(case, name):
    model, N = case
    c = oracle_case(model, N)
    B = len(c["r"]["x"])
    ns = lc.dims(model, N)[1]
    cot = lc.cotangents(model, N, B, name)
    same = c["same"]
    ref = ln.step_vjp(c["q"], c["jac"], c["r"]["x"], c["r"]["lam"], cot, ns, only=np.nonzero(same)[0])
    k = ref["x0"].shape[1]
    worst = 0.0
    for col in range(k):
        an = np.einsum("bi,bi->b", ref["x0"][:, col], c["v0"]) + np.einsum("bi,bi->b", ref["x_ref"][:, col], c["vr"])
        phi = []
        for o in (c["plus"], c["minus"]):
            p = np.zeros(B)
            for key, v in cot.items():
                if v is not None:
                    p = p + (v[:, col] * o[key] if key == "fbar" else np.einsum("bi,bi->b", v[:, col], o[key]))
            phi.append(p)
        fd = (phi[0] - phi[1]) / (2 * H_DIFF)
        err = np.abs(fd - an) / np.maximum(1.0, np.maximum(np.abs(an), np.abs(fd)))
        worst = max(worst, float(err[same].max()))
    print("LTVSENS_CPU " + json.dumps(dict(test="reference vs differences", case=lc.case_id(case), cotangents=name, compared=int(same.sum()),
                                           of=B, worst=worst, bound=FD_BOUND[case])))
    assert same.sum() >= B * 3 // 4, int(same.sum())
    assert worst <= FD_BOUND[case], worst


@pytest.mark.parametrize("model", [0, 1])
def test_inputs_activate_every_row_family_on_refined_vertices(model):
    N = lc.N_ROWS
    c = oracle_case(model, N)
    r, refined = c["r"], c["refined"]
    B = len(refined)
    nx, ns, nV, nC = lc.dims(model, N)
    fam = {name: int((r["lam"][refined][:, nV + rows] != 0).any(axis=1).sum()) for name, rows in lc.families(model, N).items()}
    slack = int((np.abs(r["x"][refined][:, 2 * N:]) > 1e-9).any(axis=1).sum())
    print("LTVSENS_CPU " + json.dumps(dict(test="inputs", case=lc.case_id((model, N)), refined=int(refined.sum()), of=B, families=fam,
                                           slack_nonzero=slack, working_set_holds=int(c["same"].sum()))))
    assert sum(len(rows) for rows in lc.families(model, N).values()) == nC
    assert refined.sum() >= B * 3 // 4, int(refined.sum())
    assert all(n >= 2 for n in fam.values()), fam
    assert slack >= 1


@pytest.mark.parametrize("model", [0, 1])
def test_infeasible_instances_fail_in_the_oracle(model):
    d = lc.infeasible_inputs(model)
    _, r, _ = oracle_step(model, lc.N_ROWS, d["x0"], d["x_ref"].reshape(lc.B_INFEASIBLE, -1), d["x_lin"], d["u_lin"])
    bad = np.zeros(lc.B_INFEASIBLE, dtype=bool)
    bad[list(lc.INFEASIBLE)] = True
    assert (r["exitflag"][bad] != 0).all() and (r["exitflag"][~bad] == 0).all(), r["exitflag"]
