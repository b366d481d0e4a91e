"""CPU tests of the closed loop's Cartesian sensor models: the new names, the restated measurement function
(tests/sensors_numpy.py) against the frame transform as a round trip, its Jacobian by dual numbers against differences, the row-by-row
update against the textbook joint update, the heading wrap at +-pi, every Python refusal with no track loaded, the refusals of the
two entries on host buffers, the filtering gain of the restated filter on a synthetic drive, and csrc/cl_sensors.h on the host under
the sanitizers against the restatement, bit for bit."""
import os
import shutil
import subprocess
import sys

import numpy as np

import estimator_numpy as en
import frame_numpy as fn
import sensors_cases as sc
import sensors_numpy as sn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _states(otr, model, seed, count):
    """Curvilinear states all over the track: |n| <= 0.6 m, |mu| <= 0.3 rad, segment joints and the wrap of the arc length included."""
    rng = np.random.default_rng(seed)
    nx = sn.nx_of(model)
    x = np.zeros((count, nx))
    x[:, 0] = rng.uniform(0.0, otr.L, count)
    x[:4, 0] = [0.0, otr.dl, otr.L - 1e-9, 3 * otr.dl - 1e-12]
    x[4, 0] = otr.L + 7.3
    x[5, 0] = -2.1
    x[:, 1] = rng.uniform(-0.6, 0.6, count); x[:, 2] = rng.uniform(-0.3, 0.3, count); x[:, 3] = rng.uniform(1.0, 20.0, count)
    x[:, 4:] = rng.uniform(-0.3, 0.3, (count, nx - 4))
    return x


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in ("fsaempc_cl_sense_batch_device", "fsaempc_cl_estimate_cart_batch_device"):
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header
    assert "} fsaempc_cl_sensors;" in header
    assert "CartesianSensors" in fm.__all__ and hasattr(fm, "CartesianSensors") and hasattr(fm._lib, "ClSensors")
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    for flag in ("--sensors", "--sensor-seed"):
        assert flag in tool
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/cl_sensors.o" in mk.split("COMMON :=")[1].split("\n")[0]      # COMMON goes into every library, the -O1 guard included
    for f in ("cl_sensors.h", "cl_sensors.hip"):
        assert os.path.exists(os.path.join(ROOT, "fsae-mpc_amd", "csrc", f))


def test_h_inverts_the_frame_transform(otrack):
    """cart_to_curv(h(x)) = x: frame_numpy's projection of the pose h gives, started 0.5 m off the true arc length, returns (s, n, mu).
    The Newton search stops at a step below 0.01 m, so s comes back to within that step's square-law remainder and n, mu with it; the
    bound 1e-4 (m, rad) is that of a converged last step of 0.01 m at the track's curvature (< 0.3 / m): 0.3 * 0.01^2 = 3e-5."""
    worst = 0.0
    for x in _states(otrack, 0, 3, 60)[6:]:
        hv = sn.h_values(otrack, x)
        s, n, mu = fn.cart_to_curv(otrack, hv[0], hv[1], hv[2], x[0] + 0.5, np.float64)
        worst = max(worst, abs(s - x[0]), abs(n - x[1]), abs(mu - x[2]))
        assert np.array_equal(hv[3:], x[3:])
    print("round trip h -> cart_to_curv: worst %.3e" % worst)
    assert worst <= 1e-4


def test_jacobian_by_duals_against_differences(otrack):
    """H from the dual numbers against Richardson-extrapolated central differences of h (estimator_numpy.fd_jacobian, step 1e-3, the
    states 0.3 .. 2.7 m into a segment so that every stencil stays inside it): 1e-8 of max(1, |H|), the differences' own error; only
    the block of rows and columns 0 .. 2 differs from the identity."""
    worst = levels = 0.0
    for model in (0, 1):
        nx = sn.nx_of(model)
        for x in _states(otrack, model, 5, 40):
            x = x.copy()
            x[0] = np.floor(x[0] / otrack.dl) * otrack.dl + 0.3 + 2.4 * ((x[0] / otrack.dl) % 1.0)
            hv, H = sn.linearise(otrack, x)
            assert np.array_equal(hv.view(np.uint64), sn.h_values(otrack, x).view(np.uint64))
            J, gap = en.fd_jacobian(lambda xx: sn.h_values(otrack, xx), x, np.full(nx, 1e-3))
            scale = max(1.0, np.abs(J).max())
            worst, levels = max(worst, np.abs(H - J).max() / scale), max(levels, gap / scale)
            rest = H.copy(); rest[:3, :3] = np.eye(3)
            assert np.array_equal(rest, np.eye(nx))
            assert H[2, 2] == 1.0 and H[0, 2] == 0.0 and H[1, 2] == 0.0 and H[2, 1] == 0.0
    print("H by duals against differences: %.3e of max(1, |H|); the two Richardson levels apart by %.3e" % (worst, levels))
    assert levels <= 1e-8 and worst <= 1e-8


def _spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T


def test_row_update_is_the_joint_update(otrack):
    """Random SPD P (condition 1 .. 100), H of random track states, random masks of unmeasured components, exact measurements (r = 0)
    included: x, P and the NIS of the row-by-row form equal K = P H' (H P H' + R)^-1 to 1e-12 relative (the bound of the same test of
    the curvilinear filter), and P stays exactly symmetric."""
    rng = np.random.default_rng(43)
    worst = 0.0
    for model in (0, 1):
        nx = sn.nx_of(model)
        xs = _states(otrack, model, 9, 40)
        for trial in range(40):
            P = _spd(rng, nx, 10.0 ** rng.uniform(0, 2)) * 10.0 ** rng.uniform(-3, 1)
            P = 0.5 * (P + P.T)
            x = xs[trial]
            h0, H = sn.linearise(otrack, x)
            y = h0 + 0.1 * rng.standard_normal(nx)
            r = 10.0 ** rng.uniform(-4, 0, nx)
            r[rng.random(nx) < 0.25] = np.inf
            if trial % 4 == 1:
                r[rng.integers(nx)] = 0.0
            if trial % 8 == 3:
                r[rng.integers(nx)] = np.nan
            if trial % 8 == 5:
                r[rng.integers(nx)] = -1.0
            if trial == 7:
                r[:] = np.inf
            xr, Pr, innov, nis = sn.row_update(x, P, y, r, h0, H)
            xj, Pj, nisj = sn.joint_update(x, P, y, r, h0, H)
            scale = max(np.abs(xj).max(), 1e-300)
            worst = max(worst, np.abs(xr - xj).max() / scale, np.abs(Pr - Pj).max() / np.abs(P).max(), abs(nis - nisj) / max(nisj, 1e-300) if nisj > 0 else abs(nis))
            assert np.array_equal(Pr, Pr.T)
            m = np.array([en.measured(v) for v in r])
            assert (innov[~m] == 0).all()
            if trial == 7:
                assert np.array_equal(xr, x) and np.array_equal(Pr, P) and nis == 0.0
    print("row-by-row against joint update: worst relative difference %.3e" % worst)
    assert worst <= 1e-12


def test_heading_wrap():
    """angdiff(h2, y2) at +-pi: the innovation of a heading across the cut is the short way round, +pi (not -pi) for a positive
    difference, and y2 + 2 pi k gives the innovation of y2."""
    pi = np.pi
    assert sn.angdiff(3.1, -3.1) == (-3.1 - 3.1 + pi) - np.floor((-6.2 + pi) / (2 * pi)) * (2 * pi) - pi
    assert abs(sn.angdiff(3.1, -3.1) - (2 * pi - 6.2)) < 1e-15 and abs(sn.angdiff(-3.1, 3.1) + (2 * pi - 6.2)) < 1e-15
    assert sn.angdiff(0.0, pi) == pi and sn.angdiff(0.0, -pi) == -pi and sn.angdiff(0.0, 3 * pi) == pi
    assert sn.angdiff(0.25, 0.25) == 0.0
    for k in (-3, -1, 1, 2):
        assert abs(sn.angdiff(0.3, 0.5 + 2 * pi * k) - 0.2) < 1e-14
    nu = sn.innovation0(np.array([1.0, 2.0, -3.1, 4.0, 5.0]), np.array([0.5, 2.5, 3.1, 4.0, 4.0]))
    assert nu[0] == 0.5 and nu[1] == -0.5 and abs(nu[2] - (2 * pi - 6.2)) < 1e-15 and nu[3] == 0.0 and nu[4] == 1.0


def test_python_options_are_checked_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
inf, nan = float("inf"), float("nan")
s5, s7 = [0.05, 0.05, 0.01, 0.1, 0.005], [0.05, 0.05, 0.01, 0.1, 0.05, 0.02, 0.005]
bad = [dict(sigma=0.1), dict(sigma=[0.1] * 4), dict(sigma=np.zeros((2, 3, 5))), dict(sigma=[0.1, 0, 0, nan, 0]), dict(sigma=[0.1, 0, 0, inf, 0]),
       dict(sigma=[0.1, 0, 0, -1e-9, 0]), dict(sigma="loud"), dict(sigma=None), dict(sigma=s5, seed=-1), dict(sigma=s5, seed=2 ** 64), dict(sigma=s5, seed=1.5),
       dict(sigma=s5, id0=-1), dict(sigma=s5, id0=True), dict(sigma=s5, id0=2 ** 63)]
for kw in bad:
    try:
        fm.CartesianSensors(**kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for CartesianSensors(%%r)" %% (kw,))
ok5, ok7 = fm.CartesianSensors(s5, seed=3, id0=10), fm.CartesianSensors(s7)
assert fm.CartesianSensors(np.full((3, 5), 0.1)).sigma.shape == (3, 5) and fm.CartesianSensors([0.0] * 7).sigma.shape == (7,)
q5, q7 = [1e-6] * 5, [1e-6] * 7
# with sensors r = None takes sigma^2 (sensor layout), and an unmeasured X is no obstacle to laps > 1
q, r, p0 = fm.Estimator(q5).resolve(None, 5, 3, 1, ok5)
assert list(r) == [v ** 2 for v in s5] and list(p0) == [v ** 2 for v in s5]
fm.Estimator(q5, r=[inf, 0.1, 0.1, 0.1, 0.1]).resolve(None, 5, 3, 2, ok5)
cart = [[0.0] * 7] * 3
wrong = [(fm.KINEMATIC, dict(sensors=ok7)),                                                   # the other model's nx
         (fm.DYNAMIC, dict(sensors=ok5)),
         (fm.KINEMATIC, dict(sensors=fm.CartesianSensors(np.full((2, 5), 0.1)))),             # per-car sigma of another batch
         (fm.KINEMATIC, dict(sensors=ok5, latency=fm.Latency(sigma=s5))),                     # two noise sources
         (fm.DYNAMIC, dict(sensors=ok7, latency=fm.Latency(delay=1, compensate=True, sigma=[0.0] * 7))),
         (fm.KINEMATIC, dict(sensors=ok5, estimator=fm.Estimator(q7))),
         (fm.KINEMATIC, dict(sensors=ok5, estimator=fm.Estimator(q5, r=np.full((4, 5), 0.1), p0=[1.0] * 5))),
         (fm.KINEMATIC, dict(sensors=s5)), (fm.KINEMATIC, dict(sensors=0.1)), (fm.DYNAMIC, dict(sensors="gps")), (fm.DYNAMIC, dict(sensors=dict(sigma=s7))),
         (fm.DYNAMIC, dict(sensors=fm.Latency(sigma=s7)))]
for model, kw in wrong:
    try:
        fm.ClosedLoop(model, 10, 0.05, None, cart, **kw)
    except ValueError:
        pass
    else:
        raise SystemExit("no ValueError for ClosedLoop(%%r)" %% (kw,))
    try:
        fm.monte_carlo(model, 10, fm.Track.load("fsg2019"), 3, 1, **kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for monte_carlo(%%r)" %% (kw,))
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_abi_refusals_on_host_buffers():
    """Every FSAEMPC_ERR_ARG case of the two entries is decided before any launch: with host buffers too, which stay untouched."""
    sc.check_abi_refusals("cpu")


def test_filtering_gain_of_the_restatement(orc, otrack):
    """The synthetic drive of sensors_cases.gain_drive (8 kinematic cars, 30 periods, truth rolled with param_numpy.psi, numpy noise of
    5 cm / 0.01 rad on the pose) through the restated projection and the restated filter (F by differences of param_numpy.psi): over
    periods 10 .. 29 the filter's RMS error in n and in mu is at most half of the projection's.  This is the choice of sigma and q the
    GPU test of the device filter stands on."""
    d = sc.gain_drive(orc, otrack)
    K, Cn, nx = d["truth"].shape
    x_proj, x_est = np.zeros((K, Cn, nx)), np.zeros((K, Cn, nx))
    r = sc.GAIN_SIGMA ** 2
    for c in range(Cn):
        st = dict(est_x=np.zeros(nx), est_P=np.zeros((nx, nx)), count=(0, 0))
        predict = lambda x, u: (sc.pn.psi(d["block"], orc, sc.GAIN_MODEL, otrack, x, u, sc.DT, sc.GAIN_INTEG),
                                en.psi_jacobian(d["block"], orc, sc.GAIN_MODEL, otrack, x, u, sc.DT, sc.GAIN_INTEG)[0])
        for k in range(K):
            x_proj[k, c], lost = sn.project(otrack, sc.GAIN_MODEL, d["y"][k, c], d["truth"][k, c, 0], d["truth"][k, c])
            assert not lost
            st = sn.period(st["est_x"], st["est_P"], st["count"], d["y"][k, c], x_proj[k, c], d["u"][k - 1, c] if k else np.zeros(2), 0, sc.GAIN_Q, r, r, 0.0,
                           predict, lambda x: sn.linearise(otrack, x))
            x_est[k, c] = st["x0_est"]
        assert st["count"] == (K, 0)
    rn, rmu = sc.gain_ratio(d["truth"], x_proj, x_est)
    print("restated filter against the projection, RMS error ratio over periods %d .. %d: n %.3f, mu %.3f" % (sc.GAIN_FROM, K - 1, rn, rmu))
    assert rn <= 0.5 and rmu <= 0.5


HOST_MAIN = r"""
// Stand-alone host program around csrc/cl_sensors.h: the spline table from a file (M, dl, then xP and yP column-major as the device
// holds them), then per line of the state file h(x) on doubles, h(x) and the columns of H on dual numbers, the exact measurement of
// the state read as a Cartesian vector and its way back; then the heading wrap on the pairs of the command line.
#include <stdio.h>
#include <stdlib.h>
#include "cl_sensors.h"
int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const int nx = atoi(argv[3]);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int M; double dl;
  if (fread(&M, sizeof(int), 1, f) != 1 || fread(&dl, sizeof(double), 1, f) != 1) return 4;
  double* xP = (double*)malloc(4 * M * sizeof(double));   // exact sizes on the heap: the sanitizers see any step outside
  double* yP = (double*)malloc(4 * M * sizeof(double));
  if (fread(xP, sizeof(double), 4 * M, f) != (size_t)(4 * M) || fread(yP, sizeof(double), 4 * M, f) != (size_t)(4 * M)) return 5;
  fclose(f);
  f = fopen(argv[2], "rb");
  if (!f) return 6;
  double* x = (double*)malloc(nx * sizeof(double));
  double* h = (double*)malloc(nx * sizeof(double));
  ClsD* xd = (ClsD*)malloc(nx * sizeof(ClsD));
  ClsD* hd = (ClsD*)malloc(nx * sizeof(ClsD));
  double* c = (double*)malloc(7 * sizeof(double));
  while (fread(x, sizeof(double), nx, f) == (size_t)nx) {
    cls_h<double>(M, dl, xP, yP, nx, x, h);
    printf("h");
    for (int i = 0; i < nx; ++i) printf(" %a", h[i]);
    printf("\n");
    for (int j = 0; j < nx; ++j) {
      for (int i = 0; i < nx; ++i) xd[i] = cls_mk(x[i], i == j ? 1.0 : 0.0);
      cls_h<ClsD>(M, dl, xP, yP, nx, xd, hd);
      printf("H");
      for (int i = 0; i < nx; ++i) printf(" %a %a", hd[i].v, hd[i].d);
      printf("\n");
    }
    cls_cart_from_y(nx, x, c);
    c[4] = 0.5 * x[3];
    cls_y_true(nx, c, h);
    printf("y");
    for (int i = 0; i < nx; ++i) printf(" %a", h[i]);
    printf("\n");
  }
  fclose(f);
  for (int a = 4; a + 1 < argc; a += 2) printf("A %a\n", cls_angdiff(strtod(argv[a], 0), strtod(argv[a + 1], 0)));
  free(xP); free(yP); free(x); free(h); free(xd); free(hd); free(c);
  return 0;
}
"""


def test_host_build_matches_numpy_under_sanitizers(tmp_path, otrack):
    """cl_sensors.h on the host, compiled with -fsanitize=address,undefined: h on doubles and on dual numbers (value and every column of
    H), the exact measurement and the heading wrap equal the restatement's bit for bit -- segment joints, the wrap of the arc length, a
    negative arc length, both models, +-pi and multiples of 2 pi; the sanitizers report nothing."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    (tmp_path / "sensors_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "sensors_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "sensors_main.cpp"), "-o", str(exe)])
    with open(tmp_path / "table.bin", "wb") as f:
        f.write(np.int32(otrack.M).tobytes()); f.write(np.float64(otrack.dl).tobytes())
        f.write(np.ascontiguousarray(np.asarray(otrack.xP, dtype=np.float64).T).tobytes())      # column-major: all P0, then P1, P2, P3
        f.write(np.ascontiguousarray(np.asarray(otrack.yP, dtype=np.float64).T).tobytes())
    pi = np.pi
    pairs = [(3.1, -3.1), (-3.1, 3.1), (0.0, pi), (0.0, -pi), (0.0, 3 * pi), (0.25, 0.25), (0.3, 0.5 + 2 * pi), (0.3, 0.5 - 6 * pi), (1.0, 1.0 + 1e-17), (-0.0, 0.0),
             (2.0, -2.5), (pi, -pi), (-pi, pi), (0.1, np.nextafter(0.1 + pi, 9.0)), (0.1, np.nextafter(0.1 - pi, -9.0))]
    hexf = lambda s: np.float64(float.fromhex(s))
    same = lambda a, b: np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))
    for model in (0, 1):
        nx = sn.nx_of(model)
        xs = _states(otrack, model, 17 + model, 48)
        xs.tofile(tmp_path / "states.bin")
        args = [repr(float(v)) for pr in pairs for v in pr]
        run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(tmp_path / "table.bin"), str(tmp_path / "states.bin"), str(nx)] + args,
                             capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
        lines = [l.split() for l in run.stdout.strip().split("\n")]
        hl = [[hexf(v) for v in l[1:]] for l in lines if l[0] == "h"]
        Hl = [[hexf(v) for v in l[1:]] for l in lines if l[0] == "H"]
        yl = [[hexf(v) for v in l[1:]] for l in lines if l[0] == "y"]
        al = [hexf(l[1]) for l in lines if l[0] == "A"]
        assert len(hl) == len(xs) and len(Hl) == nx * len(xs) and len(yl) == len(xs) and len(al) == len(pairs)
        for b, x in enumerate(xs):
            hv, H = sn.linearise(otrack, x)
            assert same(hl[b], sn.h_values(otrack, x)), (model, b)
            for j in range(nx):
                row = np.array(Hl[b * nx + j]).reshape(nx, 2)
                assert same(row[:, 0], hv) and same(row[:, 1], H[:, j]), (model, b, j)
            c = sn.cart_from_y(model, x); c[4] = 0.5 * x[3]
            assert same(yl[b], sn.y_true(model, c)), (model, b)
        assert same(al, [sn.angdiff(a, b) for a, b in pairs])
    assert al[0] > 0 and al[1] < 0 and al[2] == pi and al[3] == -pi and al[4] == pi and al[5] == 0.0
