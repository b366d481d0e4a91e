"""CPU tests of the closed loop's state estimator: the new names, argument validation before the library is touched, the
refusals of the entry on host buffers, the restated sequential update (tests/estimator_numpy.py) against the textbook joint update, the
consistency of the restated filter on a linear-Gaussian chain (mean NIS inside the band the chi-square law gives), and csrc/cl_estimator.h
on the host under the sanitizers against the restatement."""
import os
import shutil
import subprocess
import sys

import numpy as np

import estimator_cases as ec
import estimator_numpy as en

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    s = "fsaempc_cl_estimate_batch_device"
    assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header and "} fsaempc_cl_estimator;" in header
    assert "Estimator" in fm.__all__ and hasattr(fm, "Estimator") and hasattr(fm._lib, "ClEstimator")
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    for flag in ("--estimator", "--meas-var", "--unmeasured"):
        assert flag in tool
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert "$(LIBDIR)/cl_estimator.o" in mk.split("COMMON :=")[1].split("\n")[0]
    for f in ("cl_estimator.h", "cl_estimator.hip"):
        assert os.path.exists(os.path.join(ROOT, "fsae-mpc_amd", "csrc", f))


def test_python_options_are_checked_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
inf, nan = float("inf"), float("nan")
q5, q7 = [1e-4] * 5, [1e-4] * 7
bad = [dict(q=1e-4), dict(q=[1e-4] * 4), dict(q=np.zeros((2, 3, 5))), dict(q=[1e-4, 0, 0, nan, 0]), dict(q=[1e-4, 0, 0, inf, 0]), dict(q=[1e-4, 0, 0, -1e-9, 0]),
       dict(q="small"), dict(q=q5, r=[0.1] * 7), dict(q=q5, r=[0.1, nan, 0, 0, 0]), dict(q=q5, r=[0.1, -0.1, 0, 0, 0]), dict(q=q5, r=[0.1, -inf, 0, 0, 0]),
       dict(q=q5, r=0.1), dict(q=q5, r="loud"), dict(q=q5, r=[0.1] * 5, p0=[1.0] * 7), dict(q=q5, r=[0.1] * 5, p0=[1.0, 1.0, 0.0, 1.0, 1.0]),
       dict(q=q5, r=[0.1] * 5, p0=[1.0, 1.0, inf, 1.0, 1.0]), dict(q=q5, r=[0.1] * 5, p0=[1.0, 1.0, -1.0, 1.0, 1.0]), dict(q=q5, r=[0.1] * 5, p0=np.ones((3, 5))),
       dict(q=q5, r=np.full((3, 5), 0.1))]
for kw in bad:
    try:
        fm.Estimator(**kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for Estimator(%%r)" %% (kw,))
ok = fm.Estimator(q7, r=[0.1, 0.1, 0.1, 0.1, inf, inf, 0.0])
q, r, p0 = ok.resolve(None, 7, 3)
assert list(p0) == [0.1, 0.1, 0.1, 0.1, 1.0, 1.0, 1.0]
q, r, p0 = fm.Estimator(q5).resolve(fm.Latency(sigma=[0.5, 0.0, 0.1, 0.2, 0.3]), 5, 3)
assert list(r) == [0.25, 0.0, 0.1 ** 2, 0.2 ** 2, 0.3 ** 2] and list(p0) == [0.25, 1.0, 0.1 ** 2, 0.2 ** 2, 0.3 ** 2]
fm.Estimator(np.full((3, 5), 1e-4), r=np.full((3, 5), 0.1), p0=[1.0] * 5).resolve(None, 5, 3)
cart = [[0.0] * 7] * 3
noisy5, noisy7 = fm.Latency(sigma=[0.1] * 5), fm.Latency(sigma=[0.1] * 7)
wrong = [(fm.KINEMATIC, dict(estimator=fm.Estimator(q7, r=[0.1] * 7))),                      # the other model's nx
         (fm.DYNAMIC, dict(estimator=fm.Estimator(q5, r=[0.1] * 5))),
         (fm.KINEMATIC, dict(estimator=fm.Estimator(np.full((2, 5), 1e-4), r=[0.1] * 5))),      # per-car q of another batch
         (fm.KINEMATIC, dict(estimator=fm.Estimator(q5, r=np.full((4, 5), 0.1), p0=[1.0] * 5))),
         (fm.KINEMATIC, dict(estimator=fm.Estimator(q5))),                                     # r = None without a latency
         (fm.KINEMATIC, dict(estimator=fm.Estimator(q5), latency=fm.Latency(delay=1))),        # ... and with one that has no sigma
         (fm.DYNAMIC, dict(estimator=fm.Estimator(q7), latency=noisy5)),
         (fm.KINEMATIC, dict(estimator=fm.Estimator(q5, r=[inf, 0.1, 0.1, 0.1, 0.1]), laps=2)),  # laps > 1 with s unmeasured
         (fm.KINEMATIC, dict(estimator=2)), (fm.KINEMATIC, dict(estimator=dict(q=q5))), (fm.DYNAMIC, dict(estimator="on")), (fm.DYNAMIC, dict(estimator=(q7,)))]
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
    """Every FSAEMPC_ERR_ARG case of the entry is decided before any launch: with host buffers too, which stay untouched."""
    ec.check_abi_refusals("cpu")


def _spd(rng, n, cond):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (Q * np.logspace(0, -np.log10(cond), n)) @ Q.T


def test_sequential_update_is_the_joint_update():
    """Random SPD P (condition 1 .. 100: the textbook side solves with S, and its own error grows with that number), random masks of
    unmeasured components (+inf, and the device-only NaN / negative), exact measurements (r = 0) included: x, P and the NIS of the
    sequential form equal K = P H' (H P H' + R)^-1 to 1e-12 relative."""
    rng = np.random.default_rng(42)
    worst = 0.0
    for nx in (5, 7):
        for trial in range(40):
            P = _spd(rng, nx, 10.0 ** rng.uniform(0, 2)) * 10.0 ** rng.uniform(-3, 1)
            P = 0.5 * (P + P.T)
            x, z = rng.standard_normal(nx), rng.standard_normal(nx)
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
            xs, Ps, innov, nis = en.seq_update(x, P, z, r)
            xj, Pj, nisj = en.joint_update(x, P, z, r)
            scale = max(np.abs(xj).max(), 1e-300)
            worst = max(worst, np.abs(xs - xj).max() / scale, np.abs(Ps - Pj).max() / np.abs(P).max(), abs(nis - nisj) / max(nisj, 1e-300) if nisj > 0 else abs(nis))
            assert np.array_equal(Ps, Ps.T)                                   # exactly symmetric
            m = np.array([en.measured(v) for v in r])
            assert (innov[~m] == 0).all()
            exact = m & (r == 0)
            assert np.abs(xs[exact] - z[exact]).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(z).max())   # r = 0: the estimate is the measurement
    print("sequential against joint update: worst relative difference %.3e" % worst)
    assert worst <= 1e-12


def test_nis_of_a_linear_gaussian_chain():
    """x+ = F x + w, w ~ N(0, diag q), z = x + v on the measured components, v ~ N(0, diag r), x(0) ~ N(x_start, diag p0): every assumption
    of the filter holds, so the NIS of each period is chi-square with m = 4 degrees of freedom (mean m, variance 2 m) and the innovations
    of different periods are independent.  n = 200 cars x 50 periods = 10 000 samples: the mean must lie within m +- 6 sqrt(2 m / n) =
    4 +- 0.17, six standard deviations of the sample mean (derived, not tuned)."""
    rng = np.random.default_rng(20190)
    nx, cars, periods = 5, 200, 50
    F = np.array([[1.0, 0.0, 0.0, 0.05, 0.0], [0.0, 1.0, 0.4, 0.0, 0.0], [0.0, -0.1, 0.9, 0.0, 0.2], [0.0, 0.0, 0.0, 0.98, 0.0], [0.0, 0.0, 0.0, 0.0, 0.95]])
    q = np.array([1e-4, 4e-4, 1e-4, 1e-2, 1e-3]); r = np.array([2.5e-3, 2.5e-3, np.inf, 1e-2, 1e-4]); p0 = np.array([0.01, 0.04, 0.01, 0.25, 0.01])
    m = int(sum(en.measured(v) for v in r))
    sr = np.where(np.isfinite(r), np.sqrt(np.where(np.isfinite(r), r, 0.0)), 0.0)
    u = np.zeros(2)
    predict = lambda x, u_: (F @ x, F)
    total, n, resets = 0.0, 0, 0
    for car in range(cars):
        x_start = rng.standard_normal(nx)
        truth = x_start + np.sqrt(p0) * rng.standard_normal(nx)
        st = dict(est_x=np.zeros(nx), est_P=np.zeros((nx, nx)), count=(0, 0))
        for k in range(periods):
            if k > 0:
                truth = F @ truth + np.sqrt(q) * rng.standard_normal(nx)
            z = truth + sr * rng.standard_normal(nx)
            st = en.period(st["est_x"], st["est_P"], st["count"], z, x_start, u, 0, q, r, p0, 0.0, predict)
            total += st["nis"]; n += 1
        resets += st["count"][1]
        assert st["count"][0] == periods
    mean, half = total / n, 6 * np.sqrt(2 * m / n)
    print("mean NIS %.4f over %d samples, m = %d, band +- %.4f" % (mean, n, m, half))
    assert resets == 0 and n == 10000 and m == 4
    assert abs(mean - m) <= half


HOST_MAIN = r"""
// Stand-alone host program around csrc/cl_estimator.h: the re-basing on the (x, z, L, measured) quadruples of the command line, then the
// predicates on a fixed list of special values.
#include <stdio.h>
#include <stdlib.h>
#include "cl_estimator.h"
int main(int argc, char** argv) {
  if ((argc - 1) % 4 != 0) return 2;
  for (int a = 1; a + 3 < argc; a += 4) {
    double* v = (double*)malloc(3 * sizeof(double));   // exact size on the heap: the sanitizers see any step outside
    for (int i = 0; i < 3; ++i) v[i] = strtod(argv[a + i], 0);
    printf("R %.17g\n", cle_rebase(v[0], v[1], v[2], atoi(argv[a + 3])));
    free(v);
  }
  const double s[] = {0.0, -0.0, 1.0, -1.0, 4.9e-324, -4.9e-324, 1e308, INFINITY, -INFINITY, NAN};
  for (unsigned i = 0; i < sizeof(s) / sizeof(s[0]); ++i)
    printf("P %d %d %d %d %d %d %d\n", cle_finite(s[i]), cle_measured(s[i]), cle_prior_bad(s[i], 0), cle_prior_bad(s[i], 1), cle_post_bad(s[i], 0),
           cle_post_bad(s[i], 1), cle_gain_ok(s[i]));
  return 0;
}
"""
SPECIAL = [0.0, -0.0, 1.0, -1.0, 4.9e-324, -4.9e-324, 1e308, np.inf, -np.inf, np.nan]


def test_host_build_matches_numpy_under_sanitizers(tmp_path):
    """cl_estimator.h on the host, compiled with -fsanitize=address,undefined: the re-basing equals the restatement's bit for bit (z - x at
    +-L/2, at multiples of L, just beside both, L = 0, s unmeasured, a non-finite L), the predicates agree on +-0, denormals, inf and NaN; the
    sanitizers report nothing."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    (tmp_path / "estimator_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "estimator_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "estimator_main.cpp"), "-o", str(exe)])
    L = 308.53
    cases = []
    for x in (0.0, 3.25, L + 0.4, -2.0, 5 * L + 1.0):
        for dz in (0.0, 0.3, -0.3, L / 2, -L / 2, np.nextafter(L / 2, L), np.nextafter(-L / 2, -L), L, -L, 2 * L, -3 * L, L - 0.2, -L + 0.2, 1.5 * L, 2.5 * L):
            cases.append((x, x + dz, L, 1))
    cases += [(L + 0.4, 0.4, 0.0, 1), (L + 0.4, 0.4, L, 0), (L + 0.4, 0.4, -L, 1), (L + 0.4, 0.4, np.nan, 1), (L + 0.4, 0.4, np.inf, 1), (np.nan, 0.4, L, 1),
              (0.4, np.inf, L, 1), (-0.0, -0.0, L, 1)]
    args = [repr(float(v)) if i < 3 else str(v) for c in cases for i, v in enumerate(c)]
    run = subprocess.run(["timeout", "-k", "2", "20", str(exe)] + args, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    lines = run.stdout.strip().split("\n")
    got = np.array([float(l.split()[1]) for l in lines if l.startswith("R")])
    with np.errstate(all="ignore"):
        ref = np.array([en.rebase(x, z, Lc, m) for x, z, Lc, m in cases])
    nan = np.isnan(ref)
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), ref[~nan].view(np.uint64)), (got, ref)
    by = {c: g for c, g in zip(cases, got)}
    assert by[(L + 0.4, L + 0.4 - L, L, 1)] == (L + 0.4) + L * -1.0          # one lap back
    assert by[(3.25, 3.25 + L / 2, L, 1)] == 3.25 and by[(3.25, 3.25 - L / 2, L, 1)] == 3.25   # a tie moves nothing (rint to even)
    assert by[(L + 0.4, 0.4, 0.0, 1)] == L + 0.4 and by[(L + 0.4, 0.4, L, 0)] == L + 0.4 and by[(L + 0.4, 0.4, -L, 1)] == L + 0.4
    P = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("P")]
    ref_p = [[int(en.finite(v)), int(en.measured(v)), int(en.prior_bad(v, False)), int(en.prior_bad(v, True)), int(en.post_bad(v, False)),
              int(en.post_bad(v, True)), int(v > 0.0)] for v in SPECIAL]
    assert P == ref_p
    # spelled out: -0.0 is a measured variance and a legal posterior diagonal, but no legal prior diagonal; NaN and inf are never measured
    assert ref_p[1] == [1, 1, 0, 1, 0, 0, 0] and ref_p[7][:2] == [0, 0] and ref_p[9] == [0, 0, 1, 1, 1, 1, 0]
