"""CPU tests of the restatement of the closed loop's frame transform, plant and plan take-over (tests/frame_numpy.py, written from the
reference's files) and of the case tables of tests/test_frame_gpu.py (tests/frame_cases.py).  The float64 run of the restatement is
held to the oracle's C twin (oracle/ltv_oracle_plant.c) on every case the oracle can express -- it has no out-of-race rule, no hold
rules, and its segment lookup must not see a non-finite arc length -- at the tolerance the GPU tests use, max(32 e64, 1e-13 max(1,
|ref|)) per tensor and table with e64 the gap between the float64 and the long-double run; on a circle the frame transform is held to
the closed form; angdiff to a brute-force definition; and the drop rule of the GPU tests (a case leaves the value comparisons when
the two runs disagree on a discrete outcome) is capped at 2 % of a table and at none of the named edge cases.  These tests check the
reference and the inputs of the GPU tests, not the product."""
import numpy as np
import pytest

import frame_cases as fc
import frame_numpy as fn
import laps_numpy as lp

LD = np.longdouble
N = 40


@pytest.fixture(scope="module")
def track(orc, track_path):
    return orc.Track.load(track_path("fss2019"))


@pytest.fixture(scope="module")
def circle(orc):
    import fsae_mpc_amd as fm
    tr = fm.Track.from_points(*lp.circle_points(), M=lp.CIRCLE["M"])
    return orc.Track(tr.xP, tr.yP, tr.dl, tr.L)


def _tables(track, circle):
    """(table name, track, cases, target speed) of every frame table"""
    out = [(name, track, cases, fc.TARGET_VEL) for name, cases in fc.frame_tables(track).items()]
    return out + [("circle", circle, fc.circle_table(circle)[0], lp.CIRCLE["target_vel"])]


def _expressible(c):
    return bool(np.isfinite(c.cart).all() and np.isfinite(c.guess))


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_frame_restatement_against_the_oracle(orc, track, circle, model):
    """fn.pre and fn.cart_to_curv in float64 against orc.cl_pre and orc.cart_to_curv: x0 and x_ref to the table's tolerance, the lap
    check equal.  A car the restatement declares out of the race is compared on the frame transform alone (the oracle goes on with
    the car's own x0)."""
    for name, tr, cases, tv in _tables(track, circle):
        ref = fc.frame_reference(tr, cases, model, N, tv)
        worst = dict(x0=0.0, x_ref=0.0, curv=0.0)
        for b, c in enumerate(cases):
            if not _expressible(c) or ref["dropped"][b]:
                continue
            s, n, mu = fn.cart_to_curv(tr, c.cart[0], c.cart[1], c.cart[2], c.guess, np.float64)
            worst["curv"] = max(worst["curv"], float(fc.x0_error(np.array([[s, n, mu]]), np.array([orc.cart_to_curv(tr, *c.cart[:3], c.guess)])).max()))
            x0, x_ref, past = orc.cl_pre(model, N, fc.DT, tr, c.cart, c.guess, tv)
            assert (s >= tr.L) == bool(past), (name, c.name)
            if ref["finished"][b] == 2:
                continue
            assert ref["finished"][b] == past, (name, c.name)
            worst["x0"] = max(worst["x0"], float(fc.x0_error(ref["x0_64"][b:b + 1], x0[None]).max()))
            worst["x_ref"] = max(worst["x_ref"], float(np.abs(ref["x_ref_64"][b] - x_ref.T).max()))
        print("%-9s model %d  e64 x0 %.2e x_ref %.2e  tol %.2e %.2e  restatement - oracle: x0 %.2e x_ref %.2e (s, n, mu) %.2e  dropped %d of %d"
              % (name, model, ref["e64"]["x0"], ref["e64"]["x_ref"], ref["tol"]["x0"], ref["tol"]["x_ref"], worst["x0"], worst["x_ref"], worst["curv"],
                 int(ref["dropped"].sum()), len(cases)))
        assert worst["x0"] <= ref["tol"]["x0"] and worst["curv"] <= ref["tol"]["x0"] and worst["x_ref"] <= ref["tol"]["x_ref"], (name, worst, ref["tol"])


def test_plant_restatement_against_the_oracle(orc):
    """fn.plant_step, fn.f_cart_dyn and fn.integrate_cart_dyn in float64 (the reference's constants) against the oracle on the cars
    of every plant table, held or not: values to the table's tolerance, the same entries non-finite."""
    for name, cases in fc.plant_tables().items():
        ref = fc.plant_reference(cases)
        worst = dict(cart=0.0, pid=0.0, u_last=0.0, f=0.0, step=0.0)
        for b, c in enumerate(cases):
            v_ref = c.v_ref if np.isfinite(c.v_ref) else 1.0          # (the hold rules are not the oracle's: drive these cars on a finite set point)
            d_ref = c.delta_ref if np.isfinite(c.delta_ref) else 0.05
            got = fn.plant_step(None, c.cart, c.pid, v_ref, d_ref, fc.DT, np.float64)
            want = orc.plant_step(c.cart, c.pid, v_ref, d_ref, fc.DT)
            for k, g, w in zip(("cart", "pid", "u_last"), got, want):
                assert fc.same_finite_pattern(g, w), (name, c.name, k)
                worst[k] = max(worst[k], fc.finite_error(g, w))
            u = np.array([100.0 * (v_ref - c.cart[3]), d_ref])
            with np.errstate(all="ignore"):
                f, fo = fn.f_cart_dyn(None, c.cart, u, np.float64), orc.f_cart_dyn(c.cart, u)
                x, xo = fn.integrate_cart_dyn(None, c.cart, u, fc.DT / 10, np.float64), orc.integrate_cart_dyn(c.cart, u, fc.DT / 10)
            assert fc.same_finite_pattern(f, fo) and fc.same_finite_pattern(x, xo), (name, c.name)
            worst["f"] = max(worst["f"], fc.finite_error(f, fo) / max(1.0, fc.finite_error(0 * fo, fo)))
            worst["step"] = max(worst["step"], fc.finite_error(x, xo))
        print("%-9s e64 cart %.2e pid %.2e u_last %.2e  tol %.2e %.2e %.2e  restatement - oracle: %.2e %.2e %.2e  f (relative) %.2e one step %.2e  dropped %d of %d"
              % (name, ref["e64"]["cart"], ref["e64"]["pid"], ref["e64"]["u_last"], ref["tol"]["cart"], ref["tol"]["pid"], ref["tol"]["u_last"],
                 worst["cart"], worst["pid"], worst["u_last"], worst["f"], worst["step"], int(ref["dropped"].sum()), len(cases)))
        assert all(worst[k] <= ref["tol"][k] for k in ("cart", "pid", "u_last")), (name, worst, ref["tol"])
        assert worst["f"] <= 1e-13 and worst["step"] <= ref["tol"]["cart"], (name, worst)


def test_circle_closed_form(circle):
    """On the circle of laps_numpy.CIRCLE the arc length is R * angle, the offset R - r and the heading error theta - angle - pi / 2.  The
    margins are measured on the fitted table: the spline's largest distance from the circle bounds the error of n; its largest arc-length
    error, the shift of the foot point by its largest tangent error at the car's offset, and the Newton stop of 0.01 m bound that of s."""
    R = lp.CIRCLE["radius"]
    cases, s_cf, n_cf = fc.circle_table(circle)
    dev, ds, dh = fc.circle_deviation(circle)
    print("circle: L %.6f (2 pi R %.6f)  spline off the circle by %.3e m, arc length by %.3e m, tangent by %.3e rad" % (circle.L, 2 * np.pi * R, dev, ds, dh))
    for dtype in (np.float64, LD):
        for c, s_want, n_want in zip(cases, s_cf, n_cf):
            s, n, mu = fn.cart_to_curv(circle, c.cart[0], c.cart[1], c.cart[2], c.guess, dtype)
            shift = abs(n_want) * np.tan(dh) * R / (R - abs(n_want))
            print("  %-24s s - R angle %+.3e (margin %.3e)  n - (R - r) %+.3e (margin %.3e)" % (c.name, float(s) - s_want, ds + shift + 0.01, float(n) - n_want, dev))
            assert abs(float(s) - s_want) <= ds + shift + 0.01 and abs(float(n) - n_want) <= dev, c.name
            ang = np.arctan2(c.cart[1], c.cart[0])
            assert abs(float(fn.angdiff(ang + np.pi / 2, c.cart[2], dtype)) - float(mu)) <= dh + (ds + shift + 0.01) / R, c.name


def _angdiff_brute(d):
    """the representative of d + 2 pi k in (-pi, pi], +pi for a positive and -pi for a negative odd multiple of pi; in long doubles,
    pi the double MATLAB calls pi"""
    pi = LD(np.pi)
    best = None
    for k in range(-6, 7):
        r = LD(d) + 2 * pi * k
        if -pi < r <= pi or (r == -pi and d < 0):
            if r == pi and d < 0:
                continue
            best = r
    return best


def test_angdiff_against_brute_force():
    """fn.angdiff on a grid with +-pi, +-3 pi and the values within 1e-15 of them.  A difference inside [-pi, pi] comes back as the very
    bits of beta - alpha; any other to a few ulp of the difference, on the circle (within an ulp of the cut the two sides are one angle)."""
    pi = np.pi
    edges = [s * m * pi for s in (1, -1) for m in (1, 3)]
    grid = sorted(set(edges + [np.nextafter(e, 0) for e in edges] + [np.nextafter(e, 10 * e) for e in edges] + [e + d for e in edges for d in (1e-15, -1e-15)]
                      + [e * (1 + d) for e in edges for d in (1e-15, -1e-15)] + list(np.linspace(-10.0, 10.0, 401)) + [0.0, 2 * pi, -2 * pi, 6 * pi, -6 * pi]))
    for d in grid:
        for alpha in (0.0, 0.7, -2.5):
            beta = alpha + d
            for dtype in (np.float64, LD):
                diff = dtype(beta) - dtype(alpha)
                got = fn.angdiff(alpha, beta, dtype)
                want = _angdiff_brute(diff)
                assert -pi <= got <= pi, (d, alpha)
                if -pi <= diff <= pi:
                    assert got == diff, (d, alpha, got)
                err = abs(LD(got) - want)
                err = min(err, abs(err - 2 * LD(pi)))
                assert err <= 4 * np.spacing(abs(float(diff)) + pi), (d, alpha, float(got), float(want))
    for dtype in (np.float64, LD):      # the cut itself: odd multiples keep the sign of the difference
        assert fn.angdiff(0.0, pi, dtype) == dtype(pi) and fn.angdiff(0.0, -pi, dtype) == dtype(-pi)
        assert fn.angdiff(-pi, 2 * pi, dtype) == dtype(pi) and fn.angdiff(pi, -2 * pi, dtype) == dtype(-pi)      # 3 pi and -3 pi, exact sums


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_drop_cap_of_the_frame_tables(track, circle, model):
    """At most 2 % of a table may leave the value comparisons, and no named edge case (every case of every table but `ordinary`)."""
    for name, tr, cases, tv in _tables(track, circle):
        ref = fc.frame_reference(tr, cases, model, N, tv)
        dropped = [c.name for c, d in zip(cases, ref["dropped"]) if d]
        print("%-9s model %d: dropped %d of %d %s" % (name, model, len(dropped), len(cases), dropped))
        assert len(dropped) <= 0.02 * len(cases), (name, dropped)
        assert not (name in fc.NAMED and dropped), (name, dropped)


def test_drop_cap_of_the_plant_tables():
    P = fc.param_blocks()
    for name, cases in fc.plant_tables().items():
        for blocks in (None, P):
            ref = fc.plant_reference(cases, blocks)
            dropped = [c.name for c, d in zip(cases, ref["dropped"]) if d]
            print("%-9s %s: dropped %d of %d %s" % (name, "blocks" if blocks is not None else "fixed ", len(dropped), len(cases), dropped))
            assert len(dropped) <= 0.02 * len(cases), (name, dropped)
            assert name == "ordinary" or not dropped, (name, dropped)


def test_tables_reach_their_edges(track):
    """The cases do what their names say, on the long-double run: both sides of every threshold are there."""
    T = fc.frame_tables(track)
    fin = {name: fc.frame_reference(track, cases, 1, 3, fc.TARGET_VEL) for name, cases in T.items()}
    assert (fin["ordinary"]["finished"] == 0).all()
    assert fin["lap"]["finished"].tolist() == [0, 1, 1, 0, 1, 0, 1] and float(fin["lap"]["x0"][1, 0]) == track.L
    assert fin["lost"]["finished"].tolist() == [0, 2] * 6
    assert fin["blown"]["finished"].tolist() == [0, 2] * 4 + [2] * 17
    assert fin["newton"]["finished"].tolist() == [0, 0, 2, 0, 1, 0, 0, 2, 2]
    assert fin["newton"]["newton"][:8].max() < 30 and fin["newton"]["newton"][8] == 1000 and fin["newton"]["x0"][3, 0] < 0 and fin["newton"]["x0"][4, 0] > track.L
    mu = fin["heading"]["x0"][:, 2].astype(np.float64)
    assert (np.abs(np.abs(mu[:4]) - np.pi) < 2e-12).all() and mu[2] > 0 > mu[3] and (np.abs(mu[4:]) < 1e-13).all()
    for model in (0, 1):
        r = fc.frame_reference(track, T["ramp"], model, N, fc.TARGET_VEL)
        v = r["x_ref"][:, :, 3].astype(np.float64)
        up = np.array([c.cart[3] < fc.TARGET_VEL for c in T["ramp"]])
        assert up.tolist() == [True, False, False, True, False, True, True, True, False]
        assert (v[up] <= fc.TARGET_VEL).all() and (v[~up] >= fc.TARGET_VEL).all() and (np.diff(v[5]) > 0).sum() >= 38 and (np.diff(v[4]) < 0).sum() >= 13
        assert (v[3] == fc.TARGET_VEL).all() if model == 0 else v[3, 0] < fc.TARGET_VEL      # the kinematic ramp starts from hypot(vx, vy), above the target
    P = fc.param_blocks()
    pt = fc.plant_tables()
    sides = {}
    for c in pt["pid"]:
        info = {}
        fn.plant_step(None, c.cart, c.pid, c.v_ref, c.delta_ref, fc.DT, LD, info)
        sides[c.name] = info["pid"]
    first = [sides[c.name][0] for c in pt["pid"][:8]]
    assert first == [(1, 0), (-1, 0), (0, 1), (0, -1), (0, 0), (-1, 0), (0, 1), (0, 0)]
    a, b = (fc.plant_reference(pt["pid"][i:i + 1]) for i in (8, 9))      # KI = KD = 0: the output does not read the carried state, the stored state does
    assert np.array_equal(a["cart"], b["cart"]) and np.array_equal(a["u_last"], b["u_last"]) and not np.array_equal(a["pid"], b["pid"])
    slip = fc.plant_reference(pt["slip"])
    assert np.isfinite(slip["cart"][[0, 1, 3]].astype(np.float64)).all() and not np.isfinite(slip["cart"][2].astype(np.float64)).all()
    after = fn.pre(1, 3, fc.DT, fc.TARGET_VEL, track, slip["cart_64"][2], 10.0, np.float64)
    assert after[2] == 2 and (after[0] == 0).all()
    assert fc.plant_reference(pt["hold"])["held"].tolist() == [True, True, True, False, False, False, False, True, True, False, False]
    assert fc.plant_reference(pt["hold"], null_flags=True)["held"].tolist() == [True, True, False, False, False, False, False, True, True, False, False]
    assert fc.plant_reference(pt["hold"], P)["held"].tolist() == [True, True, True, False, False, False, False, True, True, True, True]
    assert [fn.block_is_bad(P[i]) for i in range(6)] == [False, False, False, False, True, True]


def test_accept_restatement():
    for nx, Nh in ((5, 3), (7, 9)):
        t = fc.accept_table(nx, Nh)
        for flags, takes in ((t["exitflag"], [True, True] + [False] * (len(t["name"]) - 2)), (None, [True] * 7 + [False] * (len(t["name"]) - 7))):
            for b in range(len(t["name"])):
                xk, uk = fn.accept(t["x_new"][b], t["u_new"][b], None if flags is None else int(flags[b]), t["x_keep"][b], t["u_keep"][b])
                src = ("x_new", "u_new") if takes[b] else ("x_keep", "u_keep")
                assert np.array_equal(xk, t[src[0]][b]) and np.array_equal(uk, t[src[1]][b]), (t["name"][b], flags is None)
