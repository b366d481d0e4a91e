"""The reference side of tests/test_sens_shapes_gpu.py, on the CPU alone: the numpy adjoint (tests/sens_numpy.py) against closed
forms on families F and E, its Hbar and Abar against Richardson-extrapolated central differences of the working-set solution map
(kkt_numpy.vertex_from_working_set) -- a shared sign or transposition error of the two implementations of the same formulas would
pass every comparison of one with the other -- and the conditions under which the GPU file demands a derivative (flag 0, refined,
independent working rows, nW <= nF, cond(K) <= 1e6), shown to hold on the oracle's vertices of F, E, S and V at qf.VJP_SHAPES.
Tests that measure print a line starting SENSSHAPES_CPU before they assert; profiles/sens_shapes/README.md records them."""
import json
import os

import numpy as np
import pytest

import kkt_numpy as kn
import qp_families as qf
import sens_numpy as sn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = sorted(os.path.join(ROOT, "tests", "golden", f) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                if f.endswith(".npz") and not f.startswith("regress_"))
B = 8
COND_MAX = 1e6
WEAK_TOL = 1e-8                # fsaempc_qp_default_opts: tol; a working-set multiplier <= tol (1 + |lambda|_inf) gives status 1
ROW_EDGE_NV = 35
ROW_EDGE_NC = (0, 1, 63, 64, 65, 255, 256, 257)     # the ballot compaction walks rows 64 at a time, the row loops stride by 256
FD_SHAPES = [(16, 16), (35, 50), (66, 33), (130, 65)]
OUT_KEYS = ("g", "lb", "ub", "lbA", "ubA", "H", "A")
R_DEPENDENT_52_70 = 1          # an instance of R (52, 70) whose duplicate rows 3 and 4 are both in the oracle's working set


def cotangents(B_, k, nV, seed):
    """The cotangent columns of group A: column 0 random xbar and fbar, column 1 random xbar with fbar = 0, column 2 (if any) all zero."""
    rng = np.random.default_rng([77, nV, seed])
    xbar = rng.standard_normal((B_, k, nV))
    fbar = rng.standard_normal((B_, k))
    if k > 1:
        fbar[:, 1] = 0.0
    if k > 2:
        xbar[:, 2] = 0.0
        fbar[:, 2] = 0.0
    return xbar, fbar


def closed_form(q, xbar, fbar):
    """The VJP of family F or E at its closed-form solution, from the dense KKT matrix transposed -- no free / pinned split, no
    equilibration: [H A_W'; A_W 0] (w, mu) = (xbar + fbar (H x + g), 0) on the rows with a multiplier (none for F: w = H^-1 xbar),
    gbar = -w + fbar x, mu on the side the sign of lambda names, Hbar and Abar by their formulas.  Same keys as sn.adjoint."""
    H, g, A, x, lam = q["H"], q["g"], q["A"], q["x_star"], q["lam_star"]
    n, m = len(g), A.shape[0]
    lamA = lam[n:]
    W = np.nonzero(lamA)[0]
    k = len(W)
    K = np.block([[H, -A[W].T], [A[W], np.zeros((k, k))]]).T
    rhs = np.concatenate([xbar + fbar * (H @ x + g), np.zeros(k)])
    sol = np.linalg.solve(K, rhs)
    sol += np.linalg.solve(K, rhs - K @ sol)
    w, muA = sol[:n], np.zeros(m)
    muA[W] = sol[n:]             # K = [H -A_W'; A_W 0] is the matrix of the forward solve (qp_families.make), K' the one above
    return dict(w=w, mu=np.concatenate([np.zeros(n), muA]), g=-w + fbar * x, lb=np.zeros(n), ub=np.zeros(n),
                lbA=np.where(lamA > 0, muA, 0.0), ubA=np.where(lamA < 0, muA, 0.0),
                H=-0.5 * (np.outer(w, x) + np.outer(x, w)) + 0.5 * fbar * np.outer(x, x),
                A=np.where((lamA != 0)[:, None], np.outer(lamA, w) - np.outer(muA, x), 0.0))


def star_working_set(q):
    return sn.working_set_rule(q["lb"], q["ub"], q["lbA"], q["ubA"], q["x_star"], q["A"], q["lam_star"])


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if np.size(b) else 0.0


def vjp_conditions(q, x, lam, flag, polished):
    """Per instance of a stacked batch q: the working set of the rule at (x, lam) and what the VJP needs of it.  Returns a list of
    dict(ws, nF, nW, rank, cond, ok, weak): ok = flag 0, full row rank on the free columns, nW <= nF and cond(K) <= 1e6."""
    out = []
    for b in range(len(q["g"])):
        ws = sn.working_set_rule(q["lb"][b], q["ub"][b], q["lbA"][b], q["ubA"][b], x[b], q["A"][b].T, lam[b])
        c = sn.conditions(q["H"][b].T, q["A"][b].T, ws)
        c["ws"] = ws
        c["independent"] = c["rank"] == c["nW"]
        c["ok"] = bool(flag[b] == 0 and c["independent"] and c["nW"] <= c["nF"] and c["cond"] <= COND_MAX)
        c["weak"] = bool((np.abs(lam[b][ws != 0]) <= WEAK_TOL * (1.0 + np.abs(lam[b]).max())).any())
        c["polished"] = bool(polished[b] > 0)
        out.append(c)
    return out


def test_family_V_is_R_without_the_duplicate():
    for nV, nC in [(35, 50), (130, 65)]:
        for inst in (0, 3):
            v, r = qf.make("V", nV, nC, inst), qf.make("R", nV, nC, inst)
            rest = np.arange(nC) != 4
            assert all(np.array_equal(v[k], r[k]) for k in ("H", "g", "lb", "ub"))
            assert all(np.array_equal(v[k][rest], r[k][rest]) for k in ("A", "lbA", "ubA"))
            assert np.array_equal(r["A"][3], r["A"][4]) and v["x_star"] is None and v["lam_star"] is None
            A = v["A"]
            assert np.linalg.matrix_rank(A[[3, 4]] / np.abs(A[[3, 4]]).max(axis=1, keepdims=True)) == 2          # a row of its own
            xs = v["lb"] + 1.0                                                                                   # lb = xs - 1, variable 3 is fixed
            xs[3] = v["lb"][3]
            scale = np.abs(A[4]).max()
            assert 1e-5 <= scale <= 1e5 and v["ubA"][4] == np.inf                                                # feasible around xs, as its neighbours
            assert 0.0 < (A[4] @ xs - v["lbA"][4]) / scale < 1.5
    a, b = qf.make("V", 52, 70, 2, ha_inst=0), qf.make("V", 52, 70, 5, ha_inst=0)
    assert np.array_equal(a["A"], b["A"]) and a["lbA"][4] != b["lbA"][4]
    assert "V" not in qf.FAMILIES                      # the tests of the forward solve are parametrised over FAMILIES
    s = qf.stack([qf.make("E", 16, 16, i) for i in range(2)])
    assert s["lam_star"].shape == (2, 32) and np.count_nonzero(s["lam_star"][0]) == 8 and not s["lam_star"][:, :16].any()
    assert not qf.batch("F", 16, 16, 2)["lam_star"].any() and "lam_star" not in qf.batch("S", 16, 16, 2)


# ---- closed forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in ("F", "E") for n, m in qf.VJP_SHAPES + (qf.SHAPES_F_ONLY if f == "F" else [])])
def test_numpy_adjoint_matches_the_closed_forms(family, nV, nC):
    """F: gbar = -H^-1 xbar + fbar x, every bound and row cotangent zero; E: (w, mu) from the dense KKT matrix transposed.
    1e-9 relative in every output (cond(K) <= 1e3: the two dense solves differ by rounding only)."""
    xbar, fbar = cotangents(2, 3, nV, 0)
    worst = 0.0
    for b in range(2):
        q = qf.make(family, nV, nC, b)
        ws = star_working_set(q)
        assert not ws[:nV].any() and np.array_equal(ws[nV:] != 0, q["lam_star"][nV:] != 0)
        if family == "E":
            kE = min(nC, nV // 2)
            assert np.count_nonzero(ws[nV:]) == kE and (ws[nV:nV + kE] == -np.sign(q["lam_star"][nV:nV + kE])).all()
            stat = q["H"] @ q["x_star"] + q["g"] - q["A"].T @ q["lam_star"][nV:]
            assert np.abs(stat).max() <= 1e-9 * max(1.0, np.abs(q["g"]).max())          # lam_star in the solver's convention
        for c in range(3):
            cf = closed_form(q, xbar[b, c], fbar[b, c])
            ad = sn.adjoint(q["H"], q["g"], q["A"], q["x_star"], q["lam_star"], ws, xbar[b, c], fbar[b, c])
            if family == "F":
                assert _rel(cf["g"], -np.linalg.solve(q["H"], xbar[b, c]) + fbar[b, c] * q["x_star"]) <= 1e-9
                assert not any(ad[key].any() for key in ("lb", "ub", "lbA", "ubA", "A"))
            for key in OUT_KEYS + ("w", "mu"):
                worst = max(worst, _rel(ad[key], cf[key]))
            if c == 2:
                assert not any(np.any(ad[key]) for key in OUT_KEYS)
    print("SENSSHAPES_CPU " + json.dumps(dict(test="closed forms", case="%s (%d,%d)" % (family, nV, nC), worst=worst)))
    assert worst <= 1e-9, worst


# ---- Hbar and Abar against differences -------------------------------------------------------------------------------------------

def _richardson(diff, h, levels):
    """Central differences at h, h/2, ... extrapolated (even error expansion); diff(t) = f(t) - f(-t)."""
    D = [diff(h / 2 ** i) / (2 * h / 2 ** i) for i in range(levels)]
    for j in range(1, levels):
        D = [(4 ** j * D[i + 1] - D[i]) / (4 ** j - 1) for i in range(len(D) - 1)]
    return D[0]


def _check_H_and_A_against_differences(H, g, A, lb, ub, lbA, ubA, x, lam, rng, tag):
    """Directions: a symmetric dH restricted to H's pattern and dA scaled entry-wise by |A| (h = 1e-4 relative to each entry).  The
    map is not affine in H and A, so the plain central difference carries truncation error (up to 7.6e-6 in A at h = 1e-4):
    extrapolation from h and h/2, from h/4 too where that misses the bound.  Returns the worst error over the bound."""
    n = len(g)
    ws = sn.working_set_rule(lb, ub, lbA, ubA, x, A, lam)
    x0, _ = kn.vertex_from_working_set(H, g, A, lb, ub, lbA, ubA, ws)
    assert np.max(np.abs(x0 - x)) <= 1e-6 * max(1.0, np.max(np.abs(x))), tag      # the given vertex is the one of its working set
    xbar, fbar = rng.standard_normal(n), 0.7
    adj = sn.adjoint(H, g, A, x0, lam, ws, xbar, fbar)
    S = rng.standard_normal((n, n))
    dH = 0.5 * (S + S.T) * np.abs(H)
    # H + h dH has to stay positive definite with room to spare, or the differences leave the smooth regime: on the families
    # (eigenvalues 1 .. 1e3) h |dH| is below a tenth of the smallest eigenvalue as it stands; the LTV fixtures at N = 40 have
    # cond(H) = 5e5 on the curved block, there dH is scaled down to the same tenth
    curved = np.diag(H) > 0
    lmin = np.linalg.eigvalsh(H[np.ix_(curved, curved)]).min()
    dH *= min(1.0, 1e3 * lmin / np.linalg.norm(dH, 2))
    dA =rng.standard_normal(A.shape) * np.abs(A)

    def diff(dHH, dAA):
        """t -> phi(+t) - phi(-t) of phi = xbar'x + fbar fval along (dHH, dAA).  The fval part is taken as
        (H xm + g)'(x+ - x-) + t/2 (x+'dH x+ + x-'dH x-), xm the mean of the two points: fval itself reaches 7e8 on a fixture with
        an active 1e8-cost slack, and the difference of two such numbers would carry 1e-7 / h of rounding."""
        def d(t):
            xp, _ = kn.vertex_from_working_set(H + t * dHH, g, A + t * dAA, lb, ub, lbA, ubA, ws)
            xm, _ = kn.vertex_from_working_set(H - t * dHH, g, A - t * dAA, lb, ub, lbA, ubA, ws)
            return xbar @ (xp - xm) + fbar * ((H @ (0.5 * (xp + xm)) + g) @ (xp - xm) + 0.5 * t * (xp @ dHH @ xp + xm @ dHH @ xm))
        return d

    worst = 0.0
    for key, f in (("H", diff(dH, 0.0 * dA)), ("A", diff(0.0 * dH, dA))):
        if key == "A" and A.shape[0] == 0:
            continue
        an = float(np.sum(adj[key] * (dH if key == "H" else dA)))
        bound = 1e-6 * max(1.0, abs(an), np.max(np.abs(xbar)))
        for levels in (2, 3):
            fd = _richardson(f, 1e-4, levels)
            if abs(fd - an) <= bound:
                break
        worst = max(worst, abs(fd - an) / bound)
        assert abs(fd - an) <= bound, (tag, key, fd, an, levels)
    return worst


@pytest.mark.parametrize("family", ["F", "E", "S", "V"])
def test_numpy_Hbar_and_Abar_match_extrapolated_differences_on_the_families(orc, family):
    rng = np.random.default_rng(17)
    worst = 0.0
    for nV, nC in FD_SHAPES:
        q = qf.vjp_batch(family, nV, nC, 2)
        if "x_star" in q:
            x, lam = q["x_star"], q["lam_star"]
        else:
            r = orc.qp_solve_batch_aux(*[q[k] for k in qf.KEYS])
            assert (r["exitflag"] == 0).all() and (r["polished"] > 0).all()
            x, lam = r["x"], r["lam"]
        for b in range(2):
            worst = max(worst, _check_H_and_A_against_differences(q["H"][b].T, q["g"][b], q["A"][b].T, q["lb"][b], q["ub"][b], q["lbA"][b],
                                                                  q["ubA"][b], x[b], lam[b], rng, (family, nV, nC, b)))
    print("SENSSHAPES_CPU " + json.dumps(dict(test="Hbar, Abar vs differences", case=family, worst_over_bound=worst)))


@pytest.mark.parametrize("path", GOLDEN[:6], ids=[os.path.basename(p) for p in GOLDEN[:6]])
def test_numpy_Hbar_and_Abar_match_extrapolated_differences_on_the_ltv_fixtures(path):
    d = np.load(path)
    rng = np.random.default_rng(7)
    worst = 0.0
    for b in range(min(2, d["g"].shape[0])):
        worst = max(worst, _check_H_and_A_against_differences(d["H"][b].T, d["g"][b], d["A"][b].T, d["lb"][b], d["ub"][b], d["lbA"][b], d["ubA"][b],
                                                              d["x"][b], d["lam"][b], rng, (os.path.basename(path), b)))
    print("SENSSHAPES_CPU " + json.dumps(dict(test="Hbar, Abar vs differences", case=os.path.basename(path), worst_over_bound=worst)))


# ---- attainability ---------------------------------------------------------------------------------------------------------------

def _attain_figures(orc, family, nV, nC):
    q = qf.vjp_batch(family, nV, nC, B)
    r = orc.qp_solve_batch_aux(*[q[k] for k in qf.KEYS])
    cs = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])
    fig = dict(test="attainability", case="%s (%d,%d)" % (family, nV, nC), first=qf.vjp_first(family, nV, nC),
               flags=np.unique(r["exitflag"]).tolist(), refined=int((r["polished"] > 0).sum()),
               dependent=int(sum(not c["independent"] for c in cs)), over=int(sum(c["nW"] > c["nF"] for c in cs)),
               cond=float(max([c["cond"] for c in cs if c["independent"] and c["nW"] <= c["nF"]] or [0.0])),
               weak=int(sum(c["weak"] for c in cs)), ok=int(sum(c["ok"] for c in cs)),
               nF=[min(c["nF"] for c in cs), max(c["nF"] for c in cs)], nW=[min(c["nW"] for c in cs), max(c["nW"] for c in cs)])
    print("SENSSHAPES_CPU " + json.dumps(fig))
    return fig, r, cs


@pytest.mark.parametrize("family,nV,nC", [(f, n, m) for f in ("F", "E", "S", "V") for n, m in qf.VJP_SHAPES])
def test_oracle_vertices_meet_the_conditions_of_the_vjp(orc, family, nV, nC):
    """Group B of the GPU file leaves no instance out: with the oracle as the forward every instance is flag 0 and refined, its
    working rows restricted to the free columns have full row rank, nW <= nF and cond(K) <= 1e6."""
    fig, r, cs = _attain_figures(orc, family, nV, nC)
    assert fig["flags"] == [0] and fig["refined"] == B, fig
    assert fig["dependent"] == 0 and fig["over"] == 0 and fig["cond"] <= COND_MAX and fig["ok"] == B, fig


@pytest.mark.parametrize("nV,nC", qf.VJP_SHAPES)
def test_family_R_has_dependent_working_rows(orc, nV, nC):
    """Recorded, not bounded: how many of 8 instances of R put both duplicate rows 3 and 4 (or otherwise dependent rows) into the
    working set -- why R gets the either/or of group C instead of a comparison on every instance."""
    fig, r, cs = _attain_figures(orc, "R", nV, nC)
    assert fig["flags"] == [0], fig


@pytest.mark.parametrize("nC", ROW_EDGE_NC)
def test_row_count_edges_conditions(orc, nC):
    """V at nV = 35 around the 64-row trips of the compaction and the 256-row stride of the row loops.  With more rows than
    variables many vertices are degenerate (nW > nF, dependent rows): group E compares as group B where the conditions hold and by
    the rules of group C elsewhere; here: flag 0 everywhere, and the conditions hold on every instance while nC <= 1."""
    fig, r, cs = _attain_figures(orc, "V", ROW_EDGE_NV, nC)
    assert fig["flags"] == [0], fig
    if nC <= 1:
        assert fig["ok"] == B and fig["refined"] == B, fig


def test_the_dependent_instance_of_the_slot_test_is_dependent(orc):
    q = qf.batch("R", 52, 70, 1, first=R_DEPENDENT_52_70)
    r = orc.qp_solve_batch_aux(*[q[k] for k in qf.KEYS])
    c = vjp_conditions(q, r["x"], r["lam"], r["exitflag"], r["polished"])[0]
    assert r["exitflag"][0] == 0 and c["ws"][52 + 3] != 0 and c["ws"][52 + 3] == c["ws"][52 + 4] and c["rank"] == c["nW"] - 1 and c["nW"] <= c["nF"]
