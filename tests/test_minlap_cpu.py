"""CPU tests of the minimum-time racing line: the restated adjoint (tests/minlap_numpy.py) against central differences
of raceline_numpy.line_profile, its lap time bit for bit that profile's, csrc/minlap.h on the host under the sanitizers against the
restatement, the conditioning of the gradient (what fixes the GPU tolerance), the vetting of every fixture tests/test_minlap_gpu.py
runs, argument validation before the library is touched and what the new entries do without a device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import minlap_cases as mc
import minlap_numpy as mn
import raceline_numpy as rn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BUILD_TOL = 1e-9      # the project's construction tolerance: test_gradient_conditioning keeps a 1e-13 input difference below 1e-11
FD_TOL = 1e-7         # of max |grad|, central differences at h = 1e-5 (measured <= 5.5e-9)
BRANCH_GAP = 1e-9     # the two sides of every vetted branch decision differ by more than this, relative
NEW = ["fsaempc_plan_line_lapgrad_batch_device", "fsaempc_plan_minlap_workspace_bytes", "fsaempc_plan_minlap_batch_device"]
# the five cases of the study and one with a parameter block of its own at grip 0.8: (track, model, N_s, N_c, v_cap, grip, block seed)
FD_CASES = [("fss2019", 1, 128, 32, 20.0, 1.0, None), ("fso2020", 1, 37, 9, 20.0, 1.0, None), ("fsg2019", 0, 500, 100, 20.0, 1.0, None),
            ("fsg2019", 0, 128, 32, 9.0, 1.0, None), ("fso2020", 0, 37, 9, 20.0, 1.0, None), ("fss2019", 1, 128, 32, 20.0, 0.8, 77)]


def _track(orc, track_path, name):
    return orc.Track.load(track_path(name))


def _block(model, seed):
    if seed is None:
        return None
    import fsae_mpc_amd as fm
    return fm.param_draws(model, [1], seed, 0.2)[0]


def test_new_names_exist():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header, s
    assert callable(fm.Plan.minlap) and callable(fm.Plan.lap_gradient)
    assert fm._lib.MINLAP_RHO == mn.RHO_DEFAULT and fm._lib.MINLAP_MAX_NS == mn.MINLAP_MAX_NS
    tool = open(os.path.join(ROOT, "tools", "closed_loop_bench.py")).read()
    assert "--minlap" in tool


def test_minlap_limits_match_the_header(tmp_path):
    from fsae_mpc_amd import _lib
    src = tmp_path / "limits.c"
    src.write_text('#include <stdio.h>\n#include "fsaempc.h"\nint main(void) {\n'
                   '  printf("%d %d\\n", FSAEMPC_MINLAP_MAX_NS, FSAEMPC_MINLAP_MAX_RHO);\n  return 0;\n}\n')
    exe = tmp_path / "limits"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert out == [_lib.MINLAP_MAX_NS, _lib.MINLAP_MAX_RHO] and _lib.MINLAP_MAX_NS >= 1024, out


@pytest.mark.parametrize("case", FD_CASES, ids=lambda c: "%s-m%d-%dx%d-cap%g-grip%g%s" % (c[:6] + ("-block" if c[6] else "",)))
def test_adjoint_against_central_differences(orc, track_path, case):
    """dT/dc of the restatement against (T(c + h e_j) - T(c - h e_j)) / 2h of raceline_numpy.line_profile's sum of t, h = 1e-5, on the
    minimum-curvature line in +-0.5; the restated T is bit for bit that sum."""
    name, model, N_s, N_c, v_cap, grip, seed = case
    otr = _track(orc, track_path, name)
    k, c, par = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c), _block(model, seed)
    res = mn.lap_gradient(model, k, otr.L, c, v_cap, grip, par)
    T = lambda x: rn.line_profile(model, k, otr.L, x, v_cap, grip, par)["t"].sum()
    assert res["T"] == T(c)                                            # the same bits
    assert np.array_equal(res["t"], rn.line_profile(model, k, otr.L, c, v_cap, grip, par)["t"])
    h = 1e-5
    fd = np.zeros(N_c)
    for j in range(N_c):
        e = np.zeros(N_c); e[j] = h
        fd[j] = (T(c + e) - T(c - e)) / (2 * h)
    err = np.abs(res["grad"] - fd).max() / np.abs(fd).max()
    print("max |grad - fd| / max |fd| %.3e, max |grad| %.3e, cells won fwd/bwd %d/%d" % (err, np.abs(fd).max(), int((res["won"] & 1).sum()), int((res["won"] & 2).sum() // 2)))
    assert err <= FD_TOL
    if v_cap < 20.0:
        assert (res["vlat"] == v_cap).sum() > N_s // 4                 # many capped cells


HOST_MAIN = r"""
// Stand-alone host program around csrc/minlap.h.  Input per case: [Ns, Nc, L, model, A_lat, grip, v_cap, U_ACC_MAX, ELL_LONG] + the
// centre-line curvature (Ns) + control points (Nc), all doubles; output: [nan flag, T] + grad (Nc).  Every buffer has its exact size
// on the heap, so the sanitizers see any step outside.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "minlap.h"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double h[9]; int cases = 0;
  while (fread(h, sizeof(double), 9, in) == 9) {
    const int Ns = (int)h[0], Nc = (int)h[1];
    std::vector<double> kap((size_t)Ns), c((size_t)Nc), work((size_t)11 * Ns), grad((size_t)Nc, -777.0);
    std::vector<int> won((size_t)Ns);
    if (fread(kap.data(), sizeof(double), kap.size(), in) != kap.size() || fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 3;
    const MlCar car{h[7], h[8]};
    double T = -777.0;
    const int rc = h[3] != 0.0 ? ml_lapgrad_host<true>(car, h[4], h[5], h[6], Ns, Nc, h[2], kap.data(), c.data(), work.data(), won.data(), &T, grad.data())
                               : ml_lapgrad_host<false>(car, h[4], h[5], h[6], Ns, Nc, h[2], kap.data(), c.data(), work.data(), won.data(), &T, grad.data());
    const double head[2] = {(double)rc, T};
    fwrite(head, sizeof(double), 2, out); fwrite(grad.data(), sizeof(double), grad.size(), out);
    ++cases;
  }
  fclose(in); fclose(out);
  printf("ran %d\n", cases);
  return 0;
}
"""


def test_host_build_matches_numpy_under_sanitizers(orc, track_path, tmp_path):
    """minlap.h on the host, compiled with -fsanitize=address,undefined: T and grad against the restatement at the construction
    tolerance on every fixture of the GPU tests, the smallest shapes (16, 8) and (37, 9), and a line that folds over a corner (NaN)."""
    import plan_numpy as pn
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    cases = []
    for case in mc.GRAD_CASES:
        otr = _track(orc, track_path, case[0])
        cases.append((otr, case[1], case[2], case[3], case[4], case[5], mc.line(orc, otr, case), None))
    otr = _track(orc, track_path, "fss2019")
    cases.append((otr, 1, 16, 8, 20.0, 1.0, 0.4 * np.sin(np.arange(8) * 0.9), None))
    cases.append((otr, 0, 37, 9, 20.0, 0.7, 0.4 * np.cos(np.arange(9) * 1.3), None))
    cases.append((otr, 1, 128, 32, 20.0, 0.8, mc.mincurv(orc, otr, 128, 32), _block(1, 77)))
    k128 = mc.kappa(orc, otr, 128)
    cases.append((otr, 1, 128, 32, 20.0, 1.0, np.full(32, 0.95 / np.abs(k128).max() * np.sign(k128[np.argmax(np.abs(k128))])), None))   # a = 0.05
    with open(tmp_path / "in.bin", "wb") as f:
        for otr, model, N_s, N_c, v_cap, grip, c, par in cases:
            cst = pn.constants(par)
            np.array([N_s, N_c, otr.L, model, pn.a_lat(model, cst, grip), grip, v_cap, cst["U_ACC_MAX"], cst["ELL_LONG"]], dtype=np.float64).tofile(f)
            np.ascontiguousarray(mc.kappa(orc, otr, N_s)).tofile(f); np.ascontiguousarray(c, dtype=np.float64).tofile(f)
    (tmp_path / "minlap_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "minlap_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), str(tmp_path / "minlap_main.cpp"), "-o", str(exe)])
    run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.strip() == "ran %d" % len(cases), (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    off = 0
    for n, (otr, model, N_s, N_c, v_cap, grip, c, par) in enumerate(cases):
        rc, T, grad = got[off], got[off + 1], got[off + 2: off + 2 + N_c]; off += 2 + N_c
        ref = mn.lap_gradient(model, mc.kappa(orc, otr, N_s), otr.L, c, v_cap, grip, par)
        if n == len(cases) - 1:
            assert rc == 1 and np.isnan(T) and np.isnan(grad).all() and np.isnan(ref["T"]) and np.isnan(ref["grad"]).all()
            continue
        assert rc == 0 and not (grad == -777.0).any()
        eT, eg = abs(T - ref["T"]) / ref["T"], np.abs(grad - ref["grad"]).max() / np.abs(ref["grad"]).max()
        print("case %d (%d, %d): T rel %.2e, grad rel %.2e" % (n, N_s, N_c, eT, eg))
        assert eT <= 1e-12 and eg <= BUILD_TOL, (n, eT, eg)
    assert off == got.size


@pytest.mark.parametrize("case", mc.GRAD_CASES + [("fss2019", 1, 500, 100, 20.0, 1.0), ("fsg2019", 0, 500, 100, 20.0, 0.7)], ids=str)
def test_gradient_conditioning(orc, track_path, case):
    """A relative perturbation of 1e-13 in the control points and the centre-line curvature moves the gradient by at most 1e-11 of
    max |grad| (measured <= 4.4e-13) and T by less: the GPU parity tolerance is the construction tolerance 1e-9."""
    name, model, N_s, N_c, v_cap, grip = case
    otr = _track(orc, track_path, name)
    k, c = mc.kappa(orc, otr, N_s), mc.line(orc, otr, case)
    ref = mn.lap_gradient(model, k, otr.L, c, v_cap, grip)
    worst = worst_T = 0.0
    for seed in range(3):
        rng = np.random.default_rng(seed)
        r2 = mn.lap_gradient(model, k * (1 + 1e-13 * rng.standard_normal(N_s)), otr.L, c * (1 + 1e-13 * rng.standard_normal(N_c)), v_cap, grip)
        worst = max(worst, np.abs(r2["grad"] - ref["grad"]).max() / np.abs(ref["grad"]).max())
        worst_T = max(worst_T, abs(r2["T"] - ref["T"]) / ref["T"])
    print("gradient moved by %.3e of max |grad|, T by %.3e" % (worst, worst_T))
    assert worst <= 1e-11 and worst_T <= 1e-12


@pytest.mark.parametrize("case", mc.GRAD_CASES, ids=str)
def test_gpu_gradient_fixtures_are_vetted(orc, track_path, case):
    """No branch decision of a fixture is a close call, so a different last bit of atan on the device cannot flip one."""
    otr = _track(orc, track_path, case[0])
    res = mc.restated(orc, otr, case)
    gaps = {kind: mn.closest_call(res["pairs"][kind]) for kind in mc.VETTED}
    print(gaps, "i0", res["i0"])
    assert np.isfinite(res["T"]) and all(g > BRANCH_GAP for g in gaps.values()), gaps
    if case == mc.WRAP_CASE:
        assert res["i0"] in (0, case[2] - 1)
    if case[4] < 20.0:
        assert (res["vlat"] == case[4]).any() and (res["vlat"] < case[4]).any()


@pytest.mark.parametrize("case", mc.STEP_CASES, ids=str)
def test_gpu_step_fixtures_are_vetted(orc, track_path, case):
    """One restated iteration from the minimum-curvature line in +-0.5 gains at least 0.05 s, the best and the second-best candidate
    differ by more than 1e-6 relative in T, and neither the start nor a candidate has a close branch decision."""
    name, model, N_s, N_c, v_cap, grip = case
    otr = _track(orc, track_path, name)
    k, c = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c)
    H, g = rn.qp(orc, otr, N_s, N_c)
    res = mc.restated(orc, otr, case)
    lo, hi = np.full(N_c, -mc.W), np.full(N_c, mc.W)
    c1, g1, T1, pick, cands = mn.iterate(orc, model, k, otr.L, H, c, res["grad"], res["T"], lo, hi, mn.RHO_DEFAULT, v_cap, grip)
    Ts = np.sort([r["T"] for r, flag, cj in cands])
    print("T %.4f -> %.4f (rho index %d), candidates %s" % (res["T"], T1, pick, [round(r["T"], 4) for r, f, cj in cands]))
    assert all(flag == 0 for r, flag, cj in cands)
    assert res["T"] - T1 >= 0.05 and pick >= 0
    assert (Ts[1] - Ts[0]) / Ts[0] > 1e-6
    assert (np.abs(c1) <= mc.W).all()
    for r, flag, cj in cands:
        full = mn.lap_gradient(model, k, otr.L, cj, v_cap, grip, want_pairs=True)
        assert all(mn.closest_call(full["pairs"][kind]) > BRANCH_GAP for kind in mc.VETTED)


def test_the_loop_never_gets_slower(orc, track_path):
    otr = _track(orc, track_path, "fso2020")
    N_s, N_c = 37, 9
    k, c = mc.kappa(orc, otr, N_s), mc.mincurv(orc, otr, N_s, N_c)
    H, g = rn.qp(orc, otr, N_s, N_c)
    c3, lap, step = mn.loop(orc, 1, k, otr.L, H, c, np.full(N_c, -mc.W), np.full(N_c, mc.W), 3)
    print(lap, step)
    assert (np.diff(lap) <= 0).all() and lap[-1] < lap[0] - 0.3 and (np.abs(c3) <= mc.W).all()
    assert all((s >= 0) == (b < a) for s, a, b in zip(step, lap[:-1], lap[1:]))


def test_minlap_validation_happens_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import numpy as np
import fsae_mpc_amd as fm
def refused(f, what):
    try:
        f()
    except ValueError:
        return
    raise SystemExit("no ValueError for %%s" %% (what,))
K = fm.KINEMATIC
refused(lambda: fm.Plan.minlap(K, None, N_s=1025, N_c=100), "N_s above the cap")
refused(lambda: fm.Plan.minlap(K, None, N_s=199, N_c=100), "N_s < 2 N_c")
refused(lambda: fm.Plan.minlap(K, None, N_c=7), "N_c = 7")
for iters in (-1, 2.5, True):
    refused(lambda: fm.Plan.minlap(K, None, iters=iters), "iters = %%r" %% (iters,))
for rho in ((), (1.0,) * 17, (1.0, 0.0), (1.0, -3.0), (float("nan"),), (float("inf"),), ("a",), 5.0):
    refused(lambda: fm.Plan.minlap(K, None, rho=rho), "rho = %%r" %% (rho,))
for margin in (-0.1, float("nan")):
    refused(lambda: fm.Plan.minlap(K, None, margin=margin), "margin = %%r" %% (margin,))
refused(lambda: fm.Plan.minlap(K, None, grip=1.5), "grip")
refused(lambda: fm.Plan.minlap(K, None, v_cap=0), "v_cap")
refused(lambda: fm.Plan.minlap(2, None), "model")
refused(lambda: fm.Plan.minlap(K, None, corridor=3), "corridor that is none")
refused(lambda: fm.Plan.minlap(K, None, N_s=128, N_c=32, c_init=np.zeros(31)), "c_init with another N_c")
refused(lambda: fm.Plan.minlap(K, None, N_s=128, N_c=32, c_init=np.zeros((3, 32)), params=np.zeros(32)), "lines with one shared block")
refused(lambda: fm.Plan.minlap(K, None, params=np.zeros(31)), "params shape")
refused(lambda: fm.Plan.lap_gradient(K, None, np.zeros(32), N_s=1025), "lap_gradient N_s above the cap")
refused(lambda: fm.Plan.lap_gradient(K, None, np.zeros(7), N_s=128), "lap_gradient N_c = 7")
refused(lambda: fm.Plan.lap_gradient(K, None, np.zeros((3, 32)), N_s=128, n_plans=2), "lap_gradient line / n_plans")
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_minlap_entries_check_their_arguments_and_compute_nothing_without_a_gpu():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    tr = fm.Track.load("fsg2019")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    p = lambda a: C.c_void_p(a.data_ptr())
    xP, yP = t(tr.xP.T), t(tr.yP.T)
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    N_s, N_c, P, K, J = 64, 16, 2, 3, 4
    line = torch.full((P * N_c,), 7.0, dtype=torch.float64)
    box = torch.full((P * N_c,), 0.5, dtype=torch.float64)
    T, grad = torch.full((P,), 7.0, dtype=torch.float64), torch.full((P * N_c,), 7.0, dtype=torch.float64)
    flag, step = torch.full((P,), 7, dtype=torch.int32), torch.full((P * K,), 7, dtype=torch.int32)
    table, tt, lap = torch.full((P * N_s * 8,), 7.0, dtype=torch.float64), torch.full((P * N_s,), 7.0, dtype=torch.float64), torch.full((P * (K + 1),), 7.0, dtype=torch.float64)
    need = L.fsaempc_plan_minlap_workspace_bytes(P, N_c, J)
    assert need > L.fsaempc_plan_raceline_workspace_bytes(P, N_c) + 5 * P * J * N_c * 8
    for n, nc, j in ((0, N_c, J), (1, 7, J), (1, 197, J), (1, N_c, 0), (1, N_c, 17)):
        assert L.fsaempc_plan_minlap_workspace_bytes(n, nc, j) == -1, (n, nc, j)
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64)
    blocks = t(np.repeat(fm.default_params(fm.DYNAMIC)[None], P, axis=0))
    shared, per = fm._lib.LtvParams(p(blocks), 0), fm._lib.LtvParams(p(blocks), 1)
    nan, inf = float("nan"), float("inf")
    ladder = lambda v: (C.c_double * len(v))(*v)
    lg = lambda model=1, L_=tr.L, par=None, n=1, ns=N_s, nc=N_c, v=20.0, gr=1.0, ln=p(line), T_=p(T), g_=p(grad), sp_=C.byref(sp): L.fsaempc_plan_line_lapgrad_batch_device(
        model, sp_, C.c_double(L_), par, n, ns, nc, ln, 1, C.c_double(v), C.c_double(gr), T_, g_, None)
    ml = lambda model=1, L_=tr.L, par=None, n=1, ns=N_s, nc=N_c, m=0.25, v=20.0, gr=1.0, k=K, rho=(100.0, 30.0, 10.0, 3.0), j=None, lo=None, hi=None, wsb=need, \
        st=p(step), rp=True: L.fsaempc_plan_minlap_batch_device(
            model, C.byref(sp), C.c_double(L_), par, n, ns, nc, C.c_double(m), C.c_double(v), C.c_double(gr), None, k, ladder(rho) if rp else None,
            len(rho) if j is None else j, None, lo, hi, p(line), p(flag), p(table), p(tt), p(lap), st, p(ws), C.c_longlong(wsb), None)
    # argument checks come first, whatever the machine
    for kw in (dict(nc=7), dict(nc=197, ns=500), dict(ns=2 * N_c - 1), dict(ns=1025, nc=100), dict(L_=0.0), dict(L_=nan), dict(L_=inf)):
        assert lg(**kw) == -1 and ml(**kw) == -1, kw
    assert lg(ns=1024, nc=100, ln=None) == -1 and lg(sp_=None) == -1 and lg(T_=None) == -1 and lg(g_=None) == -1
    for kw in (dict(v=0.0), dict(v=inf), dict(v=nan), dict(gr=0.0), dict(gr=nan), dict(gr=1.5), dict(n=0), dict(n=-3), dict(model=2), dict(par=C.byref(shared), n=2)):
        assert lg(**kw) == -1 and ml(**kw) == -1, kw
    for m in (-0.01, nan, inf, -inf):
        assert ml(m=m) == -1, m
    assert ml(k=-1) == -1 and ml(j=0) == -1 and ml(j=17) == -1 and ml(rp=False) == -1 and ml(st=None) == -1
    for rho in ((0.0,), (-1.0, 3.0), (3.0, nan), (inf,)):
        assert ml(rho=rho) == -1, rho
    assert ml(lo=p(box)) == -1 and ml(hi=p(box)) == -1                                # lo without hi, hi without lo
    assert ml(n=P, par=C.byref(per), wsb=need - 64) == -5                              # FSAEMPC_ERR_WORKSPACE
    untouched = lambda: all(bool((a == 7.0).all()) for a in (line, T, grad, table, tt, lap)) and bool((flag == 7).all()) and bool((step == 7).all()) and not bool(ws.any())
    assert untouched()
    if torch.cuda.is_available():
        return     # the rest states what happens without a device
    assert lg() == -4 and lg(n=P, par=C.byref(per)) == -4 and ml() == -4 and ml(n=P, par=C.byref(per)) == -4 and ml(k=0, st=None) == -4   # FSAEMPC_ERR_NODEVICE
    assert untouched()
