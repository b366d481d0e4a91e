"""CPU tests of the s-domain plans: properties of the numpy restatement of the planner stand-in on all three tracks,
its conditioning (what justifies the GPU tolerance), the oracle's walk on such a plan, argument validation before the library is
touched, what the new entries do without a device, the bounded walk of csrc/planner.h on the host under the sanitizers, and the
one profile body of csrc/plan_profile.h on the host, bit for bit against the three restatements."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import plan_numpy as pn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRACKS = ("fsg2019", "fss2019", "fso2020")
NS = (37, 97, 500)
NEW = ["fsaempc_plan_profile_batch_device", "fsaempc_plan_reference_batch_device", "fsaempc_cl_pre_plan_batch_device"]
_KAPPA = {}


def _kappa(orc, track_path, name, N_s):
    """curvature of the cells, computed once per (track, N_s) and left unchanged"""
    key = (name, N_s)
    if key not in _KAPPA:
        otr = orc.Track.load(track_path(name))
        k = pn.kappa_cells(orc, otr, N_s); k.setflags(write=False)
        _KAPPA[key] = (otr, k)
    return _KAPPA[key]


@pytest.mark.parametrize("name", TRACKS)
@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("N_s", NS)
def test_profile_respects_its_limits(orc, track_path, name, model, N_s):
    otr, k = _kappa(orc, track_path, name, N_s)
    v_cap = 20.0
    laps = {}
    for grip in (1.0, 0.7):
        p = pn.profile(model, k, otr.L, v_cap, grip)
        v, K, ds = p["v"], p["K"], p["ds"]
        assert (v <= p["vlat"]).all() and (v <= v_cap).all() and (v > 0).all()
        eps = 1e-12 * v_cap ** 2 / ds
        for i in range(N_s):                       # every cyclic pair, the closing pair N_s - 1 -> 0 included
            n = (i + 1) % N_s
            a = (v[n] * v[n] - v[i] * v[i]) / (2 * ds)
            assert -pn.a_x(model, p["c"], grip, p["A_lat"], v[n], K[n]) - eps <= a <= pn.a_x(model, p["c"], grip, p["A_lat"], v[i], K[i]) + eps, (i, a)
            assert a == p["table"][i, 6]
        assert (v == p["vlat"]).any() and v[p["i0"]] == p["vlat"][p["i0"]]
        assert np.array_equal(p["t"], ds / v)
        assert np.array_equal(p["table"][:, [0, 1, 3]], np.zeros((N_s, 3))) and np.array_equal(p["table"][:, 2], v)
        laps[grip] = p["t"].sum()
    assert laps[0.7] > laps[1.0]


def test_profile_orientation_figures(orc, track_path):
    """The figures of a prototype of this algorithm on fss2019 (dynamic, N_s = 500, v_cap = 20, grip 1): lap 27.89 s, v 5.55 .. 16.34."""
    otr, k = _kappa(orc, track_path, "fss2019", 500)
    p = pn.profile(1, k, otr.L, 20.0, 1.0)
    assert abs(p["t"].sum() - 27.89) < 0.05 and abs(p["v"].min() - 5.55) < 0.02 and abs(p["v"].max() - 16.34) < 0.02, (p["t"].sum(), p["v"].min(), p["v"].max())
    assert np.abs(p["table"][:, 6]).max() <= 10.0 + 1e-9


@pytest.mark.parametrize("model", [0, 1])
def test_profile_below_every_corner_speed_is_flat(orc, track_path, model):
    for name in TRACKS:
        otr, k = _kappa(orc, track_path, name, 97)
        p = pn.profile(model, k, otr.L, 3.0, 1.0)
        assert (p["vlat"] == 3.0).all() and p["i0"] == 0
        assert (p["v"] == 3.0).all() and np.array_equal(p["t"], np.full(97, p["ds"] / 3.0)) and (p["table"][:, 6] == 0).all()


@pytest.mark.parametrize("name", TRACKS)
@pytest.mark.parametrize("N_s", NS)
def test_profile_conditioning(orc, track_path, name, N_s):
    """A relative perturbation of 1e-13 in the curvature (what libm vs the device's transcendental-free spline arithmetic can differ
    by, with room) moves v by at most 1e-11 relative: the GPU parity tolerance of 1e-9 is far above it."""
    otr, k = _kappa(orc, track_path, name, N_s)
    rng = np.random.default_rng(7)
    k2 = k * (1 + 1e-13 * rng.standard_normal(N_s))
    for model in (0, 1):
        for grip in (1.0, 0.7):
            v = pn.profile(model, k, otr.L, 20.0, grip)["v"]
            v2 = pn.profile(model, k2, otr.L, 20.0, grip)["v"]
            assert (np.abs(v2 - v) / v).max() <= 1e-11


@pytest.mark.parametrize("model", [0, 1])
def test_oracle_walk_on_the_numpy_plan(orc, track_path, model):
    otr, k = _kappa(orc, track_path, "fss2019", 97)
    p = pn.profile(model, k, otr.L, 20.0, 1.0)
    rng = np.random.default_rng(3)
    s0 = np.concatenate([[0.0, otr.L, 5 * p["ds"], 3.5 * otr.L], rng.uniform(0, 2 * otr.L, 60)])
    assert s0.size == 64
    for s in s0:
        r = pn.reference(orc, model, p["table"], p["t"], p["ds"], s, 0.05, 40)
        assert r.shape == ((5, 7)[model], 40) and np.isfinite(r).all()
        assert (np.diff(r[0]) > 0).all() and r[0, 0] > s


def test_plan_validation_happens_before_the_library_is_touched():
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
for N_s in (1, 4097):
    refused(lambda: fm.Plan.profile(fm.DYNAMIC, None, N_s=N_s), "N_s = %%d" %% N_s)
for grip in (0, -1, 1.5, float("nan")):
    refused(lambda: fm.Plan.profile(fm.DYNAMIC, None, grip=grip), "grip = %%r" %% grip)
for v_cap in (0, float("inf")):
    refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, v_cap=v_cap), "v_cap = %%r" %% v_cap)
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, n_plans=0), "n_plans = 0")
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, params=np.zeros((3, 32)), n_plans=2), "params / n_plans")
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, params=np.zeros(31)), "params shape")
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, params=[0.0] * 31), "params as a list")
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, params=[[1.0] * 32, [1.0] * 31]), "ragged params")
refused(lambda: fm.Plan.profile(fm.KINEMATIC, None, params=["a"] * 32), "params that are no numbers")
elsewhere = fm.Plan.__new__(fm.Plan); elsewhere.P = 1; elsewhere.device = "cuda:1"
refused(lambda: fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, [[0.0] * 7], reference=elsewhere), "a plan on another device")
for tab, t in ((np.zeros((10, 8)), np.zeros(9)), (np.zeros((10, 7)), np.zeros(10)), (np.zeros((2, 10, 8)), np.zeros(10)),
               (np.zeros((2, 10, 8)), np.zeros((3, 10))), (np.zeros(81), np.zeros(10))):
    refused(lambda: fm.Plan.from_table(tab, t, 0.5), "table %%s t %%s" %% (tab.shape, t.shape))
refused(lambda: fm.Plan.from_table(np.zeros((10, 8)), np.zeros(10), 0.0), "ds = 0")
refused(lambda: fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, [[0.0] * 7], reference="fss2019"), "reference that is no Plan")
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_plan_struct_matches_the_header(tmp_path):
    from fsae_mpc_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fsaempc.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(fsaempc_plan), offsetof(fsaempc_plan, table), offsetof(fsaempc_plan, t), '
                   'offsetof(fsaempc_plan, N_s), offsetof(fsaempc_plan, ds), offsetof(fsaempc_plan, per_instance), FSAEMPC_PLAN_MAX_NS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = _lib.PlanTable
    assert out == [C.sizeof(S), S.table.offset, S.t.offset, S.N_s.offset, S.ds.offset, S.per_instance.offset, _lib.PLAN_MAX_NS], out


def test_plan_entries_check_their_arguments_and_compute_nothing_without_a_gpu():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("int %s(" % s) in header, s
    tr = fm.Track.load("fsg2019")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    p = lambda a: C.c_void_p(a.data_ptr())
    xP, yP = t(tr.xP.T), t(tr.yP.T)
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    N_s, N, B = 37, 10, 3
    table, tt = torch.full((2 * N_s * 8,), 7.0, dtype=torch.float64), torch.full((2 * N_s,), 7.0, dtype=torch.float64)
    blocks = t(np.repeat(fm.default_params(fm.DYNAMIC)[None], 2, axis=0))
    shared = fm._lib.LtvParams(p(blocks), 0)
    per = fm._lib.LtvParams(p(blocks), 1)
    prof = lambda model=1, L_=tr.L, par=None, n=1, ns=N_s, v=20.0, g=1.0: L.fsaempc_plan_profile_batch_device(
        model, C.byref(sp), C.c_double(L_), par, n, ns, C.c_double(v), C.c_double(g), p(table), p(tt), None)
    nan, inf = float("nan"), float("inf")
    # argument checks come first, whatever the machine
    for kw in (dict(ns=1), dict(ns=4097), dict(v=0.0), dict(v=-1.0), dict(v=inf), dict(v=nan), dict(g=0.0), dict(g=-0.5), dict(g=nan), dict(g=inf),
               dict(g=1.5), dict(L_=0.0), dict(L_=nan), dict(L_=inf), dict(n=0), dict(n=-3), dict(model=2), dict(par=C.byref(shared), n=2)):
        assert prof(**kw) == -1, kw
    assert L.fsaempc_plan_profile_batch_device(1, None, C.c_double(tr.L), None, 1, N_s, C.c_double(20.0), C.c_double(1.0), p(table), p(tt), None) == -1
    plan = fm._lib.PlanTable(p(table), p(tt), N_s, tr.L / N_s, 0)
    s0 = t(np.linspace(0, 50, B))
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        nx = fm.dims(model, N)[0]
        xr = torch.full((B * nx * N,), 7.0, dtype=torch.float64)
        x0 = torch.full((B * nx,), 7.0, dtype=torch.float64)
        fin = torch.full((B,), 7, dtype=torch.int32)
        cart, sg = t(np.zeros((B, 7))), t(np.zeros(B))
        ref = lambda pl, dt=0.05, N_=N: L.fsaempc_plan_reference_batch_device(model, pl, p(s0), C.c_double(dt), N_, B, p(xr), None)
        pre = lambda pl, dt=0.05, L_=tr.L: L.fsaempc_cl_pre_plan_batch_device(model, N, C.c_double(dt), C.c_double(L_), C.byref(sp), pl, p(cart), p(sg), B,
                                                                              p(x0), p(xr), p(fin), None)
        bad_plans = [fm._lib.PlanTable(None, p(tt), N_s, 0.5, 0), fm._lib.PlanTable(p(table), None, N_s, 0.5, 0),
                     fm._lib.PlanTable(p(table), p(tt), 0, 0.5, 0), fm._lib.PlanTable(p(table), p(tt), N_s, 0.0, 0),
                     fm._lib.PlanTable(p(table), p(tt), N_s, nan, 0)]
        assert ref(None) == -1 and pre(None) == -1
        for bp in bad_plans:
            assert ref(C.byref(bp)) == -1 and pre(C.byref(bp)) == -1
        assert ref(C.byref(plan), dt=0.0) == -1 and ref(C.byref(plan), N_=0) == -1 and pre(C.byref(plan), dt=nan) == -1 and pre(C.byref(plan), L_=0.0) == -1
        assert bool((xr == 7.0).all()) and bool((x0 == 7.0).all()) and bool((fin == 7).all())
        if torch.cuda.is_available():
            continue     # the rest states what happens without a device
        assert ref(C.byref(plan)) == -4 and pre(C.byref(plan)) == -4                      # FSAEMPC_ERR_NODEVICE
        assert prof(model=model) == -4 and prof(model=model, par=C.byref(per), n=2) == -4 and prof(model=model, par=C.byref(shared)) == -4
        assert bool((xr == 7.0).all()) and bool((x0 == 7.0).all()) and bool((fin == 7).all()) and bool((table == 7.0).all()) and bool((tt == 7.0).all())


WALK_MAIN = r"""
// Stand-alone host program around plan_walk (csrc/planner.h).  Input: cases of [Ns, ds, s0, dt, Nt, nx] + table (8 Ns) + t (Ns), all
// doubles; output: nx * Nt doubles per case.  Every buffer has its exact size on the heap, so the sanitizers see any step outside.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "planner.h"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double h[6]; int cases = 0;
  while (fread(h, sizeof(double), 6, in) == 6) {
    const int Ns = (int)h[0], Nt = (int)h[4], nx = (int)h[5];
    std::vector<double> table((size_t)Ns * 8), t((size_t)Ns), xr((size_t)nx * Nt, -777.0);
    if (fread(table.data(), sizeof(double), table.size(), in) != table.size() || fread(t.data(), sizeof(double), t.size(), in) != t.size()) return 3;
    plan_walk(table.data(), t.data(), Ns, h[1], h[2], h[3], Nt, nx, xr.data());
    fwrite(xr.data(), sizeof(double), xr.size(), out);
    ++cases;
  }
  fclose(in); fclose(out);
  printf("walked %d\n", cases);
  return 0;
}
"""


def test_walk_is_bounded_on_the_host_under_sanitizers(orc, track_path, tmp_path):
    """plan_walk on the host, compiled with -fsanitize=address,undefined: bit-equal to the oracle on a valid plan, and it returns on
    tables whose times are zero, negative, NaN or +Inf, on N_s = 2 and on s0 = NaN.  (The only place such tables are used.)"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build of the walk"
    otr, k = _kappa(orc, track_path, "fss2019", 97)
    N_s, Nt, dt = 97, 40, 0.05
    nan, inf = float("nan"), float("inf")
    cases = []   # (table, t, ds, s0, nx)
    valid = {}
    for model in (0, 1):
        p = pn.profile(model, k, otr.L, 20.0, 1.0)
        valid[model] = p
        for s0 in (0.0, otr.L, 5 * p["ds"], 3.5 * otr.L, 1234.5, 17.123):
            cases.append((p["table"], p["t"], p["ds"], s0, (5, 7)[model]))
    n_valid = len(cases)
    p = valid[1]
    hostile = []
    for mut in ("zeros", "one zero", "one negative", "one nan", "one inf"):
        t = p["t"].copy()
        if mut == "zeros": t[:] = 0.0
        elif mut == "one zero": t[3] = 0.0
        elif mut == "one negative": t[3] = -0.01
        elif mut == "one nan": t[3] = nan
        else: t[3] = inf
        for s0 in (0.0, 3 * p["ds"] + 0.01, 40.0):
            for nx in (5, 7):
                hostile.append((p["table"], t, p["ds"], s0, nx))
    two = pn.profile(1, np.array([0.05, -0.02]), 10.0, 20.0, 1.0)
    hostile += [(two["table"], two["t"], two["ds"], s0, nx) for s0 in (0.0, 7.5) for nx in (5, 7)]
    hostile += [(two["table"], np.zeros(2), two["ds"], 1.0, 7), (two["table"], np.array([1e-9, 1e-9]), two["ds"], 1.0, 7)]   # the bound itself
    hostile += [(p["table"], p["t"], p["ds"], s0, nx) for s0 in (nan, inf, -inf) for nx in (5, 7)]
    cases += hostile
    with open(tmp_path / "in.bin", "wb") as f:
        for table, t, ds, s0, nx in cases:
            np.array([t.size, ds, s0, dt, Nt, nx], dtype=np.float64).tofile(f)
            np.ascontiguousarray(table, dtype=np.float64).tofile(f); np.ascontiguousarray(t, dtype=np.float64).tofile(f)
    (tmp_path / "walk_main.cpp").write_text(WALK_MAIN)
    exe = tmp_path / "walk_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), str(tmp_path / "walk_main.cpp"), "-o", str(exe)])
    # (address and undefined-behaviour checks are what this is about; the leak check at exit needs ptrace rights a container may lack)
    run = subprocess.run(["timeout", "-k", "2", "10", str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.strip() == "walked %d" % len(cases), (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    off, rows = 0, []
    for i, (table, t, ds, s0, nx) in enumerate(cases):
        r = got[off: off + nx * Nt].reshape(Nt, nx).T; off += nx * Nt
        rows.append(r)
        assert not (r == -777.0).any(), i                                   # every entry was written
        if i < n_valid:
            r7 = orc.obtain_reference(table.reshape(-1), ds, t.size, t, s0, dt, Nt)
            if nx == 7:
                assert np.array_equal(r, r7), i
            else:
                want = pn.model_layout(0, r7)
                assert np.array_equal(r[[0, 1, 2, 4]], want[[0, 1, 2, 4]]) and (np.abs(r[3] - want[3]) <= 4 * np.spacing(want[3])).all(), i
        elif not np.isfinite(s0):
            r7 = orc.obtain_reference(table.reshape(-1), ds, t.size, t, 0.0, dt, Nt)   # walked from 0: finite placeholder rows
            assert np.isfinite(r).all() and np.array_equal(r[0], r7[0]), i
    assert off == got.size
    for i, (table, t, ds, s0, nx) in enumerate(cases):
        if (t == 0).all() or (t.size == 2 and (t == 1e-9).all()):
            # all times zero, or a horizon step that would circle the lap 2.5e7 times: the bound ends the walk, no finite row
            assert not np.isfinite(rows[i]).any(), i
            continue
        bad = ~((t > 0) & np.isfinite(t))
        if bad.any() and np.isfinite(s0):
            # one zero, negative, NaN or +Inf time in cell 3: from the horizon step that meets the cell on, the car's rows are NaN;
            # a walk that starts in it has no finite row, one that never reaches it (s0 = 40 m) is the walk on the valid plan
            first = int(np.floor(np.mod(s0, ds * t.size) / ds))
            valid_rows = pn.model_layout(nx == 7, orc.obtain_reference(table.reshape(-1), ds, t.size, valid[1]["t"], s0, dt, Nt))
            if bad[first]:
                assert np.isnan(rows[i]).all(), i
            elif s0 == 0.0:
                nan_cols = np.isnan(rows[i]).all(axis=0)
                assert nan_cols[-1] and not nan_cols[0] and np.isfinite(rows[i][:, ~nan_cols]).all(), i
                j = int(np.argmax(nan_cols))
                assert nan_cols[j:].all() and np.array_equal(rows[i][[0, 1, 2]][:, :j], valid_rows[[0, 1, 2]][:, :j]), i
            else:
                assert np.isfinite(rows[i]).all() and np.array_equal(rows[i][[0, 1, 2]], valid_rows[[0, 1, 2]]), i


PROFILE_MAIN = r"""
// Stand-alone host program around csrc/plan_profile.h.  Input per case: [Ns, model, A_lat, grip, v_cap, U_ACC_MAX, ELL_LONG, ds] + the
// centre-line curvature (Ns) + a line's curvature (Ns) and cell lengths (Ns), all doubles.  Output per case: vlat (Ns), i0, v (Ns) of
// the constant-length passes on the centre line; the same of the array-length passes on the line; i0, v, vf, won (Ns each) of the
// recorded passes on the line.  Every buffer has its exact size on the heap, so the sanitizers see any step outside.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "plan_profile.h"
template <bool DYN> static void run(const double* h, const std::vector<double>& k, const std::vector<double>& kl, const std::vector<double>& dl, FILE* out) {
  const int Ns = (int)h[0];
  const double A_lat = h[2], grip = h[3], v_cap = h[4], ds = h[7];
  const MlCar car{h[5], h[6]};
  for (int mode = 0; mode < 3; ++mode) {
    const std::vector<double>& kk = mode == 0 ? k : kl;
    std::vector<double> v((size_t)Ns), vf((size_t)Ns, -777.0), wond((size_t)Ns);
    std::vector<int> won((size_t)Ns, -777);
    for (int i = 0; i < Ns; ++i) v[i] = pp_corner_speed(kk[i], A_lat, v_cap);
    const double i0 = (double)pp_first_min(v.data(), Ns);
    if (mode < 2) fwrite(v.data(), sizeof(double), v.size(), out);
    fwrite(&i0, sizeof(double), 1, out);
    if (mode == 0) pp_passes<DYN>(car, Ns, (int)i0, A_lat, grip, kk.data(), PpConstLen{ds}, v.data(), PpNoRecord{});
    else if (mode == 1) pp_passes<DYN>(car, Ns, (int)i0, A_lat, grip, kk.data(), dl.data(), v.data(), PpNoRecord{});
    else pp_passes<DYN>(car, Ns, (int)i0, A_lat, grip, kk.data(), dl.data(), v.data(), PpRecord{vf.data(), won.data()});
    fwrite(v.data(), sizeof(double), v.size(), out);
    if (mode == 2) {
      for (int i = 0; i < Ns; ++i) wond[i] = (double)won[i];
      fwrite(vf.data(), sizeof(double), vf.size(), out); fwrite(wond.data(), sizeof(double), wond.size(), out);
    }
  }
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double h[8]; int cases = 0;
  while (fread(h, sizeof(double), 8, in) == 8) {
    const size_t Ns = (size_t)h[0];
    std::vector<double> k(Ns), kl(Ns), dl(Ns);
    if (fread(k.data(), sizeof(double), Ns, in) != Ns || fread(kl.data(), sizeof(double), Ns, in) != Ns || fread(dl.data(), sizeof(double), Ns, in) != Ns) return 3;
    if (h[1] != 0.0) run<true>(h, k, kl, dl, out); else run<false>(h, k, kl, dl, out);
    ++cases;
  }
  fclose(in); fclose(out);
  printf("ran %d\n", cases);
  return 0;
}
"""


def test_profile_header_matches_the_restatements_bit_for_bit_under_sanitizers(orc, track_path, tmp_path):
    """csrc/plan_profile.h on the host, compiled with -ffp-contract=off and -fsanitize=address,undefined: corner speeds, the first
    minimum and the two passes.  Constant length on the centre line against plan_numpy.profile (vlat, i0, v), array length on a line
    against raceline_numpy.line_profile (vlat, i0, v), the recorded variant against minlap_numpy.lap_gradient (i0, v, vf, won).  Only
    + * / sqrt fmin fmax fabs take part, correctly rounded on both sides: equality of the bits, no tolerance."""
    import minlap_numpy as mn
    import raceline_numpy as rn
    import fsae_mpc_amd as fm
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build of the profile"
    NC = {16: 8, 37: 9, 97: 24}
    # (track, N_s, model, v_cap, grip, block)
    cases = [(name, N_s, model, 20.0, 1.0, None) for name in ("fss2019", "fsg2019") for N_s in (16, 37, 97) for model in (0, 1)]
    cases += [("fss2019", 97, model, 20.0, 0.8, fm.param_draws(model, [1], 77, 0.2)[0]) for model in (0, 1)]
    cases += [("fss2019", 97, model, 3.0, 1.0, None) for model in (0, 1)]     # every cell ties
    want = []
    with open(tmp_path / "in.bin", "wb") as f:
        for name, N_s, model, v_cap, grip, par in cases:
            otr, k = _kappa(orc, track_path, name, N_s)
            c = 0.4 * np.sin(np.arange(NC[N_s]) * 0.9)
            p = pn.profile(model, k, otr.L, v_cap, grip, par)
            lp = rn.line_profile(model, k, otr.L, c, v_cap, grip, par)
            lg = mn.lap_gradient(model, k, otr.L, c, v_cap, grip, par)
            assert "v" in lp and "vf" in lg, (name, N_s)                       # (no folding line among the cases)
            want.append((p, lp, lg))
            np.array([N_s, model, p["A_lat"], grip, v_cap, p["c"]["U_ACC_MAX"], p["c"]["ELL_LONG"], p["ds"]], dtype=np.float64).tofile(f)
            for a in (k, lp["kl"], lp["dl"]):
                np.ascontiguousarray(a, dtype=np.float64).tofile(f)
    (tmp_path / "profile_main.cpp").write_text(PROFILE_MAIN)
    exe = tmp_path / "profile_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), str(tmp_path / "profile_main.cpp"), "-o", str(exe)])
    run = subprocess.run(["timeout", "-k", "2", "10", str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.strip() == "ran %d" % len(cases), (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    off = 0

    def take(n):
        nonlocal off
        off += n
        return got[off - n: off]

    for case, (p, lp, lg) in zip(cases, want):
        N_s, v_cap = case[1], case[3]
        for ref in (p, lp):
            vlat, i0, v = take(N_s), take(1)[0], take(N_s)
            assert np.array_equal(vlat, ref["vlat"]) and i0 == ref["i0"] and np.array_equal(v, ref["v"]), case
            if v_cap == 3.0:
                assert i0 == 0 and (vlat == 3.0).all() and (v == 3.0).all(), case
        i0, v, vf, won = take(1)[0], take(N_s), take(N_s), take(N_s)
        assert i0 == lg["i0"] and np.array_equal(v, lg["v"]) and np.array_equal(vf, lg["vf"]) and np.array_equal(won, lg["won"]), case
        assert np.array_equal(v, lp["v"]), case                                # recording changes nothing
    assert off == got.size
