"""CPU tests of the closed loop's cone-based localisation: the new names, the restated cone rows (tests/cone_loc_numpy.py)
against differences and against dual numbers of the composite x -> (rho, beta), the row-by-row update over own and cone rows against the
textbook joint update, the bearing wrap at +-pi, the selection rule on hand-made maps, a channel with +inf variance, every Python refusal
with no track loaded, the refusals of the two entries on host buffers, the view counts the GPU tests stand on, localising without a pose
measurement on the synthetic drive with the restated filter, and csrc/cl_cone_loc.h on the host under the sanitizers against the
restatement, bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np

import cone_loc_cases as cc
import cone_loc_numpy as cn
import estimator_numpy as en
import sensors_numpy as sn

ROOT = cc.ROOT


def _states(otr, model, seed, count):
    """Curvilinear states 0.3 .. 2.7 m into a spline segment: |n| <= 0.6 m, |mu| <= 0.3 rad"""
    rng = np.random.default_rng(seed)
    nx = sn.nx_of(model)
    x = np.zeros((count, nx))
    x[:, 0] = np.floor(rng.uniform(0.0, otr.L, count) / otr.dl) * otr.dl + rng.uniform(0.3, 2.7, count)
    x[:, 1] = rng.uniform(-0.6, 0.6, count); x[:, 2] = rng.uniform(-0.3, 0.3, count); x[:, 3] = rng.uniform(1.0, 20.0, count)
    x[:, 4:] = rng.uniform(-0.3, 0.3, (count, nx - 4))
    return x


def _cone_near(rng, hv, lo=3.0, hi=15.0):
    """A map position lo .. hi m from the pose hv, anywhere around it"""
    rad, ang = rng.uniform(lo, hi), rng.uniform(-np.pi, np.pi)
    return hv[0] + rad * np.cos(ang), hv[1] + rad * np.sin(ang)


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in ("fsaempc_cl_cone_sense_batch_device", "fsaempc_cl_estimate_cones_batch_device"):
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header
    assert "} fsaempc_cl_cone_sensor;" in header and "#define FSAEMPC_CONE_OBS_MAX 16" in header and fm.CONE_OBS_MAX == 16 == cn.OBS_MAX
    assert "ConeSensor" in fm.__all__ and hasattr(fm, "ConeSensor") and hasattr(fm._lib, "ClConeSensor")
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    for flag in ("--cone-sensor", "--cone-k", "--unmeasured-pose"):
        assert flag in tool
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/cl_cone_loc.o" in mk.split("COMMON :=")[1].split("\n")[0]      # COMMON goes into every library
    for f in ("cl_cone_loc.h", "cl_cone_loc.hip"):
        assert os.path.exists(os.path.join(ROOT, "fsae-mpc_amd", "csrc", f))


def test_rows_against_differences_and_duals(otrack):
    """The restated rows G = g Hr against (a) the dual numbers pushed through h and the polar formulas -- the derivative of the very
    formulas: 1e-12 of max(1, |J|), a few roundings of entries of size |J| apart -- and (b) Richardson-extrapolated central differences of
    the composite (estimator_numpy.fd_jacobian, step 1e-3, states inside a segment, cones 3 .. 15 m away so that the stencil's error
    stays at the differences' own): 1e-8 of max(1, |J|), the bound of the same test of h in 6s.  The columns >= 3 are zero."""
    rng = np.random.default_rng(71)
    worst_d = worst_f = levels = 0.0
    for model in (0, 1):
        nx = sn.nx_of(model)
        for x in _states(otrack, model, 5 + model, 30):
            hv, H = sn.linearise(otrack, x)
            mx, my = _cone_near(rng, hv)
            G, nu0, rho_hat = cn.rows(hv[0], hv[1], hv[2], H[:3, :3], mx, my, 0.0, 0.0)
            val = cn.composite_values(otrack, x, mx, my)
            assert rho_hat == val[0] and abs(nu0[0] + val[0]) == 0.0 and abs(nu0[1] + val[1]) < 1e-15      # nu0 = z - (rho^, beta^) at z = 0
            J = cn.composite_jacobian(otrack, x, mx, my)
            assert (J[:, 3:] == 0).all()
            scale = max(1.0, np.abs(J).max())
            worst_d = max(worst_d, np.abs(G - J[:, :3]).max() / scale)

            def f(xx):
                v = cn.composite_values(otrack, xx, mx, my)
                v[1] = val[1] + sn.angdiff(val[1], v[1])          # (continuous across the cut at +-pi)
                return v
            Jf, gap = en.fd_jacobian(f, x, np.full(nx, 1e-3))
            worst_f, levels = max(worst_f, np.abs(J - Jf).max() / scale), max(levels, gap / scale)
    print("cone rows: against the duals %.3e, against differences %.3e of max(1, |J|); the two Richardson levels apart by %.3e" % (worst_d, worst_f, levels))
    assert worst_d <= 1e-12
    assert levels <= 1e-8 and worst_f <= 1e-8


def _spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T


def test_row_update_is_the_joint_update(otrack):
    """Random SPD P (condition 1 .. 100), H of random track states, 0 .. 6 cones 2 .. 15 m away, random masks of unmeasured own
    components and cone channels (+inf), an id outside the map: x, P and the NIS of the row-by-row form over own and cone rows equal
    K = P H' (H P H' + R)^-1 on the stacked rows to 1e-12 relative (the project's bound for the same statement in 6s), P stays exactly
    symmetric, and the rows counted are the rows stacked."""
    rng = np.random.default_rng(44)
    worst = 0.0
    for model in (0, 1):
        nx = sn.nx_of(model)
        xs = _states(otrack, model, 9, 40)
        for trial in range(40):
            P = _spd(rng, nx, 10.0 ** rng.uniform(0, 2)) * 10.0 ** rng.uniform(-3, 0)
            P = 0.5 * (P + P.T)
            x = xs[trial]
            h0, H = sn.linearise(otrack, x)
            y = h0 + 0.1 * rng.standard_normal(nx)
            r = 10.0 ** rng.uniform(-4, 0, nx)
            r[rng.random(nx) < 0.25] = np.inf
            if trial % 5 == 2:
                r[:3] = np.inf                                   # no pose measurement: the cones alone carry the pose
            r_cone = 10.0 ** rng.uniform(-4, -2, 2)
            if trial % 6 == 1:
                r_cone[rng.integers(2)] = np.inf
            cones = []
            for k in range(trial % 7):
                mx, my = _cone_near(rng, h0, 2.0, 15.0)
                rho, beta = cn.composite_values(otrack, x, mx, my)
                cones.append((k, (mx, my), rho + 0.05 * rng.standard_normal(), sn.angdiff(0.0, beta + 0.01 * rng.standard_normal())))
            if trial % 7 == 6:
                cones[2] = (-1, None, cones[2][2], cones[2][3])
            o = cn.row_update(x, P, y, r, h0, H, cones, r_cone)
            xj, Pj, nisj = cn.joint_update(x, P, y, r, h0, H, cones, r_cone)
            scale = max(np.abs(xj).max(), 1e-300)
            worst = max(worst, np.abs(o["x"] - xj).max() / scale, np.abs(o["P"] - Pj).max() / np.abs(P).max(),
                        abs(o["nis"] - nisj) / max(nisj, 1e-300) if nisj > 0 else abs(o["nis"]))
            assert np.array_equal(o["P"], o["P"].T)
            assert o["rows"] == len(cn.stacked(x, y, r, h0, H, cones, r_cone)[1])
    print("row-by-row over own and cone rows against the joint update: worst relative difference %.3e" % worst)
    assert worst <= 1e-12


def test_bearing_wrap():
    """A cone straight behind the car: the bearing is +-pi, its noisy value is wrapped into [-pi, pi], and the innovation of a bearing
    across the cut is the short way round."""
    pi = np.pi
    rho, beta = cn.polar(-5.0, 1e-9, 0.0, 0.0, 0.0)
    assert rho == 5.0 and abs(beta - pi) < 1e-9 and beta <= pi
    rho, beta = cn.polar(-5.0, -1e-9, 0.0, 0.0, 0.0)
    assert abs(beta + pi) < 1e-9 and beta >= -pi
    assert cn.polar(0.0, 3.0, 0.0, 0.0, pi / 2)[1] == 0.0 and abs(cn.polar(3.0, 0.0, 0.0, 0.0, pi / 2)[1] + pi / 2) < 1e-15
    hit = 0
    for g in range(40):                                           # the noise pushes some of the draws over the cut
        det, rm, bm = cn.detect(7, 3, 5, g, 5.0, pi - 1e-3, 0.05, 0.01, 1.0)
        assert det and -pi <= bm <= pi
        hit += bm < 0
    assert 0 < hit < 40
    G, nu0, rho_hat = cn.rows(0.0, 0.0, 0.0, np.eye(3), -5.0, 0.5, 5.0, -(pi - 0.05))          # beta^ just below +pi, beta_m just above -pi
    beta_hat = cn.polar(-5.0, 0.5, 0.0, 0.0, 0.0)[1]
    assert beta_hat > 3.0 and abs(nu0[1] - (2 * pi - beta_hat - (pi - 0.05))) < 1e-14 and 0 < nu0[1] < 0.2
    assert np.array_equal(G[1], [0.5 / rho_hat ** 2, 5.0 / rho_hat ** 2, -1.0]) and np.array_equal(G[0], [5.0 / rho_hat, -0.5 / rho_hat, 0.0])


def test_selection_rule():
    """Hand-made maps around a car at the origin heading along x: none in view, exactly k_max, more than k_max (the nearest are kept,
    in order), and one position in both lists (equal ranges: the smaller index first)."""
    kw = dict(r_min=0.5, r_max=15.0, fov=2 * np.pi / 3, sigma=(0.0, 0.0), p_detect=1.0, seed=1)
    pose = (0.0, 0.0, 0.0)
    behind = np.array([[-3.0, 0.0], [-5.0, 1.0], [0.1, 0.0], [30.0, 0.0], [1.0, 4.0]])        # behind, too near, too far, outside the fov
    o = cn.sense_car(behind, np.zeros((0, 2)), pose, 0, 0, k_max=4, **kw)
    assert o["n"] == 0 and o["seen"] == 0 and (o["ids"] == -1).all() and (o["z"] == 0).all()
    left = np.array([[6.0, 1.0], [2.0, 1.0], [10.0, 1.0]]); right = np.array([[4.0, -1.0], [8.0, -1.0], [-4.0, -1.0]])
    o = cn.sense_car(left, right, pose, 0, 0, k_max=5, **kw)       # 5 in view (right[2] is behind): exactly k_max
    assert o["n"] == 5 and o["seen"] == 5 and list(o["ids"]) == [1, 3, 0, 4, 2]
    assert np.array_equal(o["z"][:, 0], np.sqrt(np.array([5.0, 17.0, 37.0, 65.0, 101.0])))          # sigma = 0 copies the true range
    o = cn.sense_car(left, right, pose, 0, 0, k_max=3, **kw)       # more than k_max: the three nearest
    assert o["n"] == 3 and o["seen"] == 5 and list(o["ids"]) == [1, 3, 0]
    o = cn.sense_car(left, right, pose, 0, 0, k_max=8, **kw)       # fewer than k_max: -1 and 0 past the count
    assert o["n"] == 5 and list(o["ids"]) == [1, 3, 0, 4, 2, -1, -1, -1] and (o["z"][5:] == 0).all()
    dup_l = np.array([[6.0, 0.5], [3.0, 0.5]]); dup_r = np.array([[3.0, 0.5], [6.0, 0.5], [4.0, 0.0]])
    o = cn.sense_car(dup_l, dup_r, pose, 0, 0, k_max=5, **kw)      # ids 1 and 2, 0 and 3 share a position
    assert list(o["ids"]) == [1, 2, 4, 0, 3] and o["z"][0, 0] == o["z"][1, 0] and o["z"][3, 0] == o["z"][4, 0]
    assert cn.select([2.0, 1.0, 2.0, 1.0], [True, True, True, False], 2) == ([1, 0], 3)
    # detection thins the candidates out, and a finished car sees nothing
    many = np.stack([np.linspace(1.0, 14.0, 60), np.zeros(60)], axis=1)
    o = cn.sense_car(many, np.zeros((0, 2)), pose, 4, 9, k_max=16, **dict(kw, p_detect=0.5))
    assert 15 < o["seen"] < 45 and o["n"] == 16 and (np.diff(o["z"][:, 0]) > 0).all()
    o = cn.sense_car(many, np.zeros((0, 2)), pose, 4, 9, k_max=16, finished=True, **kw)
    assert o["n"] == 0 and o["seen"] == 0 and (o["ids"] == -1).all()


def test_an_infinite_variance_applies_no_row(otrack):
    """r_cone = (+inf, v) is a bearing-only camera: the range rows change nothing and their innovations are 0; both +inf is the update of
    the own rows alone, bit for bit."""
    rng = np.random.default_rng(3)
    x = _states(otrack, 0, 2, 1)[0]
    h0, H = sn.linearise(otrack, x)
    P = 0.01 * _spd(rng, 5, 10.0); P = 0.5 * (P + P.T)
    y, r = h0 + 0.05, np.full(5, 0.01)
    cones = []
    for k in range(4):
        mx, my = _cone_near(rng, h0)
        rho, beta = cn.composite_values(otrack, x, mx, my)
        cones.append((k, (mx, my), rho + 0.1, beta + 0.02))
    both = cn.row_update(x, P, y, r, h0, H, cones, [0.01, 1e-4])
    cam = cn.row_update(x, P, y, r, h0, H, cones, [np.inf, 1e-4])
    off = cn.row_update(x, P, y, r, h0, H, cones, [np.inf, np.inf])
    xo, Po, inn, nis = sn.row_update(x, P, y, r, h0, H)
    assert both["rows"] == 13 and cam["rows"] == 9 and off["rows"] == 5
    assert (cam["cone_innov"][:4, 0] == 0).all() and (cam["cone_innov"][:4, 1] != 0).all() and (cam["G"][:, 0] == 0).all()
    assert np.array_equal(off["x"], xo) and np.array_equal(off["P"], Po) and off["nis"] == nis and (off["cone_innov"] == 0).all()
    assert not np.array_equal(cam["x"], xo) and not np.array_equal(both["x"], cam["x"])


def test_view_counts_on_the_centre_line(otrack):
    """What the GPU sense cases stand on: with r_max = 20 m the poses of cone_loc_cases see between 8 and 19 cones of fsg2019 each (so
    k_max = 16 truncates some cars and not others), and for every sense case no candidate lies within 1e-9 of the view's edges and no two
    candidates of a car have ranges within 1e-9 of each other unless their positions are identical."""
    left, right = cc.cone_map()
    cart = cc.poses(otrack)
    kw = dict(cc.SENSOR, seed=cc.SEED)
    wide = cn.sense(left, right, cart, 1000, 17, **dict(kw, r_max=20.0))
    print("cones in view at r_max = 20: %d .. %d" % (wide["seen"].min(), wide["seen"].max()))
    assert wide["seen"].min() >= 8 and wide["seen"].max() <= 19 and (wide["seen"] > 16).any() and (wide["seen"] < 16).any()
    assert cc.margins_ok(wide["cand"], 0.5, 20.0, kw["fov"])
    for over in (dict(), dict(p_detect=0.7), dict(k_max=3)):
        o = cn.sense(left, right, cart, 1000, 17, **dict(kw, **over))
        assert cc.margins_ok(o["cand"], kw["r_min"], kw["r_max"], kw["fov"]) and (o["n"] > 0).all()
    sl, sr = cc.synthetic_map(cart)
    o = cn.sense(sl, sr, cart, 1000, 17, **kw)
    assert cc.margins_ok(o["cand"], kw["r_min"], kw["r_max"], kw["fov"]) and (o["seen"] > 16).any() and o["n"].min() >= 1


def test_python_options_are_checked_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
inf, nan = float("inf"), float("nan")
L, R = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]), np.array([[1.0, -2.0], [3.0, -4.0]])
bad = [dict(left=0.1), dict(left=[[1.0, 2.0, 3.0]]), dict(left=np.zeros((2, 3, 2))), dict(left="cones"), dict(left=np.zeros((513, 2))), dict(right=np.zeros((600, 2))),
       dict(left=np.zeros((0, 2)), right=np.zeros((0, 2))),
       dict(r_min=0.0), dict(r_min=-1.0), dict(r_min=nan), dict(r_min=15.0), dict(r_min=20.0), dict(r_max=inf), dict(r_max=nan), dict(r_max="far"),
       dict(fov=0.0), dict(fov=-1.0), dict(fov=6.3), dict(fov=nan), dict(fov=inf), dict(fov=None),
       dict(sigma=0.1), dict(sigma=[0.1]), dict(sigma=[0.1, -1e-9]), dict(sigma=[nan, 0.1]), dict(sigma=[0.1, inf]), dict(sigma="loud"), dict(sigma=[0.1] * 3),
       dict(p_detect=-0.1), dict(p_detect=1.1), dict(p_detect=nan), dict(p_detect=None),
       dict(k_max=0), dict(k_max=17), dict(k_max=-1), dict(k_max=2.0), dict(k_max=True),
       dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(id0=-1), dict(id0=True), dict(id0=2 ** 63),
       dict(map_left=L), dict(map_right=R), dict(map_left=L[:2], map_right=R), dict(map_left=L, map_right=np.zeros((3, 2))),
       dict(map_left=np.zeros((4, 3, 2)), map_right=R), dict(map_left=np.zeros((4, 3, 2)), map_right=np.zeros((5, 2, 2))), dict(map_left=np.zeros((4, 2, 2)), map_right=np.zeros((4, 2, 2))),
       dict(r=0.1), dict(r=[0.1]), dict(r=[0.1, -1.0]), dict(r=[nan, 0.1]), dict(r="tight")]
for kw in bad:
    try:
        fm.ConeSensor(**dict(dict(left=L, right=R), **kw))
    except ValueError:
        continue
    raise SystemExit("no ValueError for ConeSensor(%%r)" %% (kw,))
ok = fm.ConeSensor(L, R, seed=3, id0=10)
assert list(ok.r) == [0.05 ** 2, 0.01 ** 2] and ok.map_left is ok.left and ok.k_max == 16 and ok.fov == 2 * np.pi / 3 and ok.r_max == 15.0 and ok.r_min == 0.5
cam = fm.ConeSensor(L, R, r=[inf, 1e-4], fov=2 * np.pi, k_max=1, p_detect=0.0, sigma=[0.0, 0.0])
assert cam.r[0] == inf
per = fm.ConeSensor(L, R, map_left=np.zeros((4, 3, 2)), map_right=np.zeros((4, 2, 2)))
one = fm.ConeSensor(L, np.zeros((0, 2)))
s5 = [0.05, 0.05, 0.01, 0.1, 0.005]
sens, est = fm.CartesianSensors(s5), fm.Estimator([1e-6] * 5, r=[inf, inf, inf, 0.01, 0.01], p0=[1.0] * 5)
cart = [[0.0] * 7] * 3
wrong = [dict(cones=ok), dict(cones=ok, sensors=sens), dict(cones=ok, estimator=fm.Estimator([1e-6] * 5, r=[0.1] * 5)),      # without sensors, without estimator
         dict(cones=per, sensors=sens, estimator=est),                                                                  # a per-car map of another batch
         dict(cones=L, sensors=sens, estimator=est), dict(cones="lidar", sensors=sens, estimator=est), dict(cones=sens, sensors=sens, estimator=est),
         dict(cones=dict(left=L, right=R), sensors=sens, estimator=est)]
for kw in wrong:
    try:
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, cart, **kw)
    except ValueError:
        pass
    else:
        raise SystemExit("no ValueError for ClosedLoop(%%r)" %% (kw,))
    try:
        fm.monte_carlo(fm.KINEMATIC, 10, fm.Track.load("fsg2019"), 3, 1, **kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for monte_carlo(%%r)" %% (kw,))
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_abi_refusals_on_host_buffers():
    """Every refusal of the two entries is decided before any launch: with host buffers too, which stay untouched."""
    cc.check_abi_refusals("cpu")


def test_localising_without_a_pose_measurement(orc, otrack):
    """The synthetic drive of sensors_cases.gain_drive with the pose rows off (r = +inf on X, Y, psi) and the first prior 0.3 m off in n
    and 0.05 rad off in mu, through the restated cone sensor and the restated filter: over periods 10 .. 29 the RMS error in n and in mu
    with cones is at most 0.75 of the same filter's without (6s's bar for "the filter helps") -- with room: the GPU test of the device
    chain stands on these figures (DESIGN.md 6t records them)."""
    res = cc.localise_restated(orc, otrack)
    print("restated filter, pose unmeasured: RMS error with cones / without, periods %d .. %d: n %.4f (%.4f / %.4f m), mu %.4f (%.5f / %.5f rad)"
          % ((cc.sc.GAIN_FROM, cc.sc.GAIN_PERIODS - 1, res["ratio"][0]) + res["rms_n"] + (res["ratio"][1],) + res["rms_mu"]))
    assert res["ratio"][0] <= 0.5 and res["ratio"][1] <= 0.5
    assert res["resets"] == 0 and res["cones_min"] >= 2


HOST_MAIN = r"""
// Stand-alone host program around csrc/cl_cone_loc.h: a cone map and poses from a file, then per pose and cone the polar coordinates,
// the view test and the draws, the selection, and the two rows of the first kept observations at the pose with a given Hr.
#include <stdio.h>
#include <stdlib.h>
#include "cl_cone_loc.h"
int main(int argc, char** argv) {
  if (argc < 10) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int n = 0, np = 0;
  if (fread(&n, sizeof(int), 1, f) != 1 || fread(&np, sizeof(int), 1, f) != 1) return 4;
  double* cone = (double*)malloc(2 * n * sizeof(double));   // exact sizes on the heap: the sanitizers see any step outside
  double* pose = (double*)malloc(3 * np * sizeof(double));
  double* hr = (double*)malloc(9 * np * sizeof(double));
  if (fread(cone, sizeof(double), 2 * n, f) != (size_t)(2 * n) || fread(pose, sizeof(double), 3 * np, f) != (size_t)(3 * np) ||
      fread(hr, sizeof(double), 9 * np, f) != (size_t)(9 * np)) return 5;
  fclose(f);
  const double r_min = strtod(argv[2], 0), r_max = strtod(argv[3], 0), fov = strtod(argv[4], 0), sr = strtod(argv[5], 0), sb = strtod(argv[6], 0),
               pd = strtod(argv[7], 0);
  const int k_max = atoi(argv[8]);
  const unsigned long long seed = strtoull(argv[9], 0, 10);
  double* rho = (double*)malloc(n * sizeof(double));
  double* rm = (double*)malloc(n * sizeof(double));
  double* bm = (double*)malloc(n * sizeof(double));
  int* cand = (int*)malloc(n * sizeof(int));
  int* ids = (int*)malloc(k_max * sizeof(int));
  for (int b = 0; b < np; ++b) {
    const double* p = pose + 3 * b;
    for (int g = 0; g < n; ++g) {
      double beta;
      clc_polar(cone[2 * g], cone[2 * g + 1], p[0], p[1], p[2], rho[g], beta);
      const int view = clc_in_view(rho[g], beta, r_min, r_max, fov);
      const int det = clc_detect(seed, 100 + b, 7 + b, g, rho[g], beta, sr, sb, pd, rm[g], bm[g]);
      if (det != clc_detected(seed, 100 + b, 7 + b, g, pd)) return 6;
      cand[g] = view && det;
      printf("P %a %a %d %d %a %a\n", rho[g], beta, view, det, rm[g], bm[g]);
    }
    int seen = 0;
    const int kept = clc_select(n, rho, cand, k_max, ids, &seen);
    printf("S %d %d", kept, seen);
    for (int k = 0; k < k_max; ++k) printf(" %d", ids[k]);
    printf("\n");
    double Hr[3][3];
    for (int i = 0; i < 3; ++i) for (int k = 0; k < 3; ++k) Hr[i][k] = hr[9 * b + 3 * i + k];
    for (int k = 0; k < kept && k < 3; ++k) {
      double G[2][3], nu0[2], rho_hat;
      clc_rows(p[0] + 0.25, p[1] - 0.125, p[2] + 0.0625, Hr, cone[2 * ids[k]], cone[2 * ids[k] + 1], rm[ids[k]], bm[ids[k]], G, nu0, rho_hat);
      printf("R %a %a %a %a %a %a %a %a %a\n", G[0][0], G[0][1], G[0][2], G[1][0], G[1][1], G[1][2], nu0[0], nu0[1], rho_hat);
    }
  }
  free(cone); free(pose); free(hr); free(rho); free(rm); free(bm); free(cand); free(ids);
  return 0;
}
"""


def test_host_build_matches_numpy_under_sanitizers(tmp_path, otrack):
    """cl_cone_loc.h on the host, compiled with -fsanitize=address,undefined: range, bearing, view, detection, the noisy observation, the
    selection and the rows equal the restatement's bit for bit (the restatement calls math.atan2, and the libm the program links); the
    sanitizers report nothing.  Cases: the map of fsg2019 with one cone doubled in the other list, poses on the track, two sensors."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    (tmp_path / "cone_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "cone_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "cone_main.cpp"), "-o", str(exe)])
    left, right = cc.cone_map()
    right = np.concatenate([right, left[5:6]])                  # one position in both lists
    cones = np.concatenate([left, right])
    cart = cc.poses(otrack, 12, seed=5)
    rng = np.random.default_rng(8)
    Hr = np.eye(3)[None] + 0.1 * rng.standard_normal((len(cart), 3, 3))
    with open(tmp_path / "cases.bin", "wb") as f:
        f.write(np.int32(len(cones)).tobytes()); f.write(np.int32(len(cart)).tobytes())
        f.write(np.ascontiguousarray(cones).tobytes()); f.write(np.ascontiguousarray(cart[:, :3]).tobytes()); f.write(np.ascontiguousarray(Hr).tobytes())
    hexf = lambda s: np.float64(float.fromhex(s))
    same = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))
    seed = 2 ** 40 + 5
    for r_min, r_max, fov, sr, sb, pd, k_max in ((0.5, 15.0, 2 * np.pi / 3, 0.05, 0.01, 1.0, 16), (1.0, 25.0, 2 * np.pi, 0.0, 0.02, 0.6, 5)):
        args = [repr(float(v)) for v in (r_min, r_max, fov, sr, sb, pd)] + [str(k_max), str(seed)]
        run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(tmp_path / "cases.bin")] + args, capture_output=True, text=True,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
        lines = [l.split() for l in run.stdout.strip().split("\n")]
        it = iter(lines)
        kept_any = 0
        for b, c in enumerate(cart):
            rho, cand, noisy = np.zeros(len(cones)), np.zeros(len(cones), dtype=bool), {}
            for g in range(len(cones)):
                l = next(it)
                assert l[0] == "P"
                rr, bb = cn.polar(cones[g, 0], cones[g, 1], c[0], c[1], c[2])
                view = cn.in_view(rr, bb, r_min, r_max, fov)
                det, rm, bm = cn.detect(seed, 100 + b, 7 + b, g, rr, bb, sr, sb, pd)
                assert same([hexf(l[1]), hexf(l[2]), hexf(l[5]), hexf(l[6])], [rr, bb, rm, bm]) and int(l[3]) == view and int(l[4]) == det, (b, g)
                rho[g], cand[g], noisy[g] = rr, view and det, (rm, bm)
            ids, seen = cn.select(rho, cand, k_max)
            l = next(it)
            assert l[0] == "S" and int(l[1]) == len(ids) and int(l[2]) == seen and [int(v) for v in l[3:]] == ids + [-1] * (k_max - len(ids)), b
            kept_any += len(ids)
            for k in ids[:3]:
                l = next(it)
                G, nu0, rho_hat = cn.rows(c[0] + 0.25, c[1] - 0.125, c[2] + 0.0625, Hr[b], cones[k, 0], cones[k, 1], noisy[k][0], noisy[k][1])
                assert l[0] == "R" and same([hexf(v) for v in l[1:]], list(G.ravel()) + list(nu0) + [rho_hat]), (b, k)
        assert next(it, None) is None and kept_any > 3 * len(cart)
