"""CPU tests of the imperfect closed loop: the restated generator (tests/latency_numpy.py) against the published
known-answer vectors of Philox4x32-10, csrc/cl_latency.h on the host under the sanitizers against the restatement (words exactly, normals
to 1e-14, the slot schedule exactly), the statistics of the draws, the slot schedule on tagged plans, and argument validation before the
library is touched."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import latency_cases as lc
import latency_numpy as ln

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ["fsaempc_cl_noise_batch_device", "fsaempc_cl_observe_batch_device", "fsaempc_cl_history_slot"]
# (seed, id, step) of the host program: small values, seed >= 2^32, id >= 2^32, step = 2^32 - 1, all three at once
TRIPLES = [(0, 0, 0), (1, 2, 3), (2 ** 40 + 3, 100, 7), (2 ** 32, 5, 0), (7, 2 ** 32, 1), (7, 2 ** 45 + 11, 2), (9, 4, 2 ** 32 - 1),
           (2 ** 64 - 1, 2 ** 63 - 1, 2 ** 32 - 1)]
PERIODS = 12


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header, s
    for name in ("Latency", "cl_noise", "CL_MAX_DELAY"):
        assert name in fm.__all__ and hasattr(fm, name)
    m = re.search(r"#define\s+FSAEMPC_CL_MAX_DELAY\s+(\d+)", header)
    assert m and int(m.group(1)) == fm.CL_MAX_DELAY == ln.MAX_DELAY == 4
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    for flag in ("--delay", "--compensate", "--noise", "--noise-seed"):
        assert flag in tool


def test_philox_known_answers():
    for ctr, key, out in ln.KAT:
        assert ln.philox(ctr, key) == out, (ctr, key)


HOST_MAIN = r"""
// Stand-alone host program around csrc/cl_latency.h: the words and normals of the (seed, id, step) triples on the command line, then the
// slot schedule for delay 0 .. FSAEMPC_CL_MAX_DELAY over the given number of periods (per period: the slot the plan is written to, the
// slot the plant reads, the slots of the predictor's inputs).
#include <stdio.h>
#include <stdlib.h>
#include "cl_latency.h"
int main(int argc, char** argv) {
  if (argc < 2 || (argc - 2) % 3 != 0) return 2;
  const int periods = atoi(argv[1]);
  for (int a = 2; a + 2 < argc; a += 3) {
    const unsigned long long seed = strtoull(argv[a], 0, 10), id = strtoull(argv[a + 1], 0, 10), step = strtoull(argv[a + 2], 0, 10);
    uint32_t w[8];
    cll_words(seed, id, step, 0, w); cll_words(seed, id, step, 1, w + 4);
    double* z = (double*)malloc(8 * sizeof(double));   // exact size on the heap: the sanitizers see any step outside
    cll_draws(seed, id, step, z);
    printf("W");
    for (int i = 0; i < 8; ++i) printf(" %08x", w[i]);
    printf("\nZ");
    for (int i = 0; i < 8; ++i) printf(" %.17g", z[i]);
    printf("\n");
    free(z);
  }
  for (int d = 0; d <= FSAEMPC_CL_MAX_DELAY; ++d)
    for (long long k = 0; k < periods; ++k) {
      printf("S %d %lld %d %d", d, k, cll_slot(d, k, 0), cll_slot(d, k, d));
      for (int j = 0; j < d; ++j) printf(" %d", cll_slot(d, k, d - j));
      printf("\n");
    }
  printf("O %.17g %.17g %.17g %.17g\n", cll_observe(-0.0, 0.0, 1.5), cll_observe(2.0, 0.25, -1.5), cll_observe(3.0, -1.0, 1.0), cll_observe(4.0, NAN, 1.0));
  return 0;
}
"""


def test_host_build_matches_numpy_under_sanitizers(tmp_path):
    """cl_latency.h on the host, compiled with -fsanitize=address,undefined: the words equal the restatement's exactly, the normals to
    1e-14 relative (same libm family, no cancellation in the map), the slot schedule exactly; the sanitizers report nothing."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    (tmp_path / "latency_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "latency_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           str(tmp_path / "latency_main.cpp"), "-o", str(exe)])
    args = [str(v) for t in TRIPLES for v in t]
    run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(PERIODS)] + args, capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    lines = run.stdout.strip().split("\n")
    W = [l.split()[1:] for l in lines if l.startswith("W")]
    Z = [l.split()[1:] for l in lines if l.startswith("Z")]
    S = [[int(v) for v in l.split()[1:]] for l in lines if l.startswith("S")]
    assert len(W) == len(Z) == len(TRIPLES)
    worst = 0.0
    for (seed, cid, step), w, z in zip(TRIPLES, W, Z):
        ref_w = ln.words(seed, cid, step, 0) + ln.words(seed, cid, step, 1)
        assert [int(v, 16) for v in w] == list(ref_w), (seed, cid, step)
        ref_z, got = ln.draws8(seed, cid, step), np.array([float(v) for v in z])
        worst = max(worst, float(np.max(np.abs(got - ref_z) / np.abs(ref_z))))
    print("normals: worst relative difference %.3e" % worst)
    assert worst <= 1e-14
    ref_s = [[d, k, ln.slot(d, k, 0), ln.slot(d, k, d)] + [ln.slot(d, k, d - j) for j in range(d)]
             for d in range(ln.MAX_DELAY + 1) for k in range(PERIODS)]
    assert S == ref_s
    o = [float(v) for v in [l for l in lines if l.startswith("O")][0].split()[1:]]
    assert o == [0.0, 2.0 + 0.25 * -1.5, 3.0, 4.0] and np.signbit(o[0])       # sigma 0, negative, NaN: a copy (-0.0 kept)


def test_draw_statistics():
    """The 2 * 10^5 draws of 25 000 ids x 1 step x 8 normals: |mean| <= 4 / sqrt(n), |var - 1| <= 4 sqrt(2 / n), nothing beyond 6.8 (the
    map's ceiling is sqrt(2 * 33 * ln 2) = 6.76); changing any one of seed, id, step changes all eight values."""
    seed, step = 2 ** 40 + 3, 5
    z = np.array([ln.draws8(seed, cid, step) for cid in range(25000)]).ravel()
    n = z.size
    assert n == 200000 and np.isfinite(z).all()
    print("mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e), max |z| %.3f" % (z.mean(), 4 / np.sqrt(n), z.var() - 1, 4 * np.sqrt(2 / n), np.abs(z).max()))
    assert abs(z.mean()) <= 4 / np.sqrt(n)
    assert abs(z.var() - 1) <= 4 * np.sqrt(2 / n)
    assert np.abs(z).max() <= 6.8
    base = ln.draws8(seed, 17, step)
    for other in (ln.draws8(seed + 1, 17, step), ln.draws8(seed + 2 ** 32, 17, step), ln.draws8(seed, 18, step), ln.draws8(seed, 17 + 2 ** 32, step),
                  ln.draws8(seed, 17, step + 1)):
        assert (other != base).all()
    # a car's draws do not depend on the batch it sits in
    assert np.array_equal(ln.noise(7, 5, seed, 100, step), ln.noise(7, 8, seed, 97, step)[3:])
    assert np.array_equal(ln.noise(5, 4, seed, 3, step), ln.noise(7, 4, seed, 3, step)[:, :5])


def test_slot_schedule_on_tagged_plans():
    """d = 0 .. 4 over 12 periods: the slot the plant reads in period k holds plan k - d ("initial" for k < d), the predictor's j-th
    input is from plan k - d + j, and the newest plan never lands on a slot still to be read."""
    for d in range(ln.MAX_DELAY + 1):
        plant, pred = ln.schedule(d, PERIODS)
        for k in range(PERIODS):
            assert plant[k] == (k - d if k >= d else "initial"), (d, k)
            assert pred[k] == [(k - d + j if k - d + j >= 0 else "initial") for j in range(d)], (d, k)
            assert all(0 <= ln.slot(d, k, lag) <= d for lag in range(d + 1))
            assert len({ln.slot(d, k, lag) for lag in range(d + 1)}) == d + 1   # the d + 1 plans in flight sit in d + 1 different slots


def test_history_slot_entry_is_the_restated_formula():
    import fsae_mpc_amd as fm
    L = fm.lib()
    for d in range(ln.MAX_DELAY + 1):
        for k in (0, 1, 2, 5, 11, 2 ** 32 - 1, 2 ** 40):
            for lag in range(d + 1):
                assert L.fsaempc_cl_history_slot(d, k, lag) == ln.slot(d, k, lag), (d, k, lag)
    for bad in ((-1, 0, 0), (5, 0, 0), (2, -1, 0), (2, 3, 3), (2, 3, -1)):
        assert L.fsaempc_cl_history_slot(*bad) == -1, bad


def test_abi_refusals_on_host_buffers():
    """Every FSAEMPC_ERR_ARG case of the two device entries is decided before any launch: with host buffers too, which stay untouched."""
    lc.check_abi_refusals("cpu")


def test_python_options_are_checked_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
inf, nan = float("inf"), float("nan")
bad = [dict(delay=-1), dict(delay=5), dict(delay=1.5), dict(delay="1"), dict(delay=True), dict(compensate=True), dict(delay=0, compensate=True),
       dict(delay=1, compensate=2), dict(sigma=[0.1] * 4), dict(sigma=np.zeros((2, 3, 5))), dict(sigma=0.1), dict(sigma=[0.1, 0, 0, nan, 0]),
       dict(sigma=[0.1, 0, 0, inf, 0]), dict(sigma=[0.1, 0, 0, -0.1, 0]), dict(sigma="loud"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0),
       dict(id0=-1), dict(id0=0.5)]
for kw in bad:
    try:
        fm.Latency(**kw)
    except ValueError:
        continue
    raise SystemExit("no ValueError for Latency(%%r)" %% (kw,))
ok = fm.Latency(delay=4, compensate=True, sigma=np.zeros(5), seed=2 ** 64 - 1, id0=2 ** 40)
assert ok.engaged and not fm.Latency().engaged and fm.Latency(sigma=[0] * 7).engaged and fm.Latency(delay=1).engaged
cart = [[0.0] * 7] * 3
wrong = [(fm.KINEMATIC, fm.Latency(sigma=[0.1] * 7)), (fm.DYNAMIC, fm.Latency(sigma=[0.1] * 5)), (fm.KINEMATIC, fm.Latency(sigma=np.zeros((2, 5)))),
         (fm.DYNAMIC, fm.Latency(sigma=np.zeros((4, 7)))), (fm.KINEMATIC, 2), (fm.KINEMATIC, dict(delay=1)), (fm.DYNAMIC, "on"), (fm.DYNAMIC, (1, True))]
for model, lat in wrong:
    try:
        fm.ClosedLoop(model, 10, 0.05, None, cart, latency=lat)
    except ValueError:
        pass
    else:
        raise SystemExit("no ValueError for ClosedLoop(latency = %%r)" %% (lat,))
    try:
        fm.monte_carlo(model, 10, fm.Track.load("fsg2019"), 3, 1, latency=lat)
    except ValueError:
        continue
    raise SystemExit("no ValueError for monte_carlo(latency = %%r)" %% (lat,))
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)
