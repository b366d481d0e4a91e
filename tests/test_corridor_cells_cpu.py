"""CPU tests of the cell-wise corridor rows of the racing line: the restatement tests/corridor_cells_numpy.py against
literals and against the line's own evaluation, csrc/raceline.h's rl_offset_row on the host under the sanitizers against the
restatement, the oracle's solution of every QP tests/test_corridor_cells_gpu.py demands, the new symbols and what the new entries
refuse without a device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import corridor_cells_cases as cases
import corridor_cells_numpy as ccn
import raceline_numpy as rn
from kkt_numpy import kkt_certificate

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KKT_TOL = 1e-6        # the tolerance of tests/test_gpu_parity.py
NEW = ["fsaempc_plan_raceline_cells_workspace_bytes", "fsaempc_plan_raceline_cells_batch_device", "fsaempc_corridor_line_rows_device"]
ROW_SHAPES = [(16, 8), (40, 8), (48, 17), (37, 9), (64, 16), (500, 100)]


def test_restatement_against_literals():
    """(N_s, N_c) = (16, 8): two cells per knot span, u = 0 and u = 1/2."""
    at_knot = np.array([1.0, 4.0, 1.0, 0.0]) / 6.0
    mid = np.array([0.125, 2.875, 2.875, 0.125]) / 6.0
    for i, first, w in ((0, 7, at_knot), (1, 7, mid), (2, 0, at_knot), (3, 0, mid), (12, 5, at_knot), (13, 5, mid), (14, 6, at_knot), (15, 6, mid)):
        got_first, got_w = ccn.row(i, 16, 8)
        assert got_first == first and np.array_equal(got_w, w), (i, got_first, got_w)
    B = ccn.matrix(16, 8)
    # rows that wrap the start of the lap: j_i = 0 (cells 0, 1) starts in the last column, j_i >= N_c - 2 (cells 12 .. 15) ends in the first ones
    want = np.zeros((16, 8))
    want[0, [7, 0, 1]] = at_knot[:3]
    want[1, [7, 0, 1, 2]] = mid
    want[12, [5, 6, 7]] = at_knot[:3]
    want[13, [5, 6, 7, 0]] = mid
    want[14, [6, 7, 0]] = at_knot[:3]
    want[15, [6, 7, 0, 1]] = mid
    for i in (0, 1, 12, 13, 14, 15):
        assert np.array_equal(B[i], want[i]), (i, B[i])
    assert np.array_equal(B[5], np.roll(want[1], 2))       # (cell 5: j = 2, the columns 1 .. 4)


@pytest.mark.parametrize("N_s,N_c", ROW_SHAPES)
def test_rows_are_the_line_s_own_evaluation(N_s, N_c):
    """B c is raceline_numpy.offsets(c)[0] bit for bit; the rows are non-negative, hold four entries in distinct columns and sum to
    one within 2 ulp."""
    B = ccn.matrix(N_s, N_c)
    rng = np.random.default_rng(N_s * 1000 + N_c)
    for _ in range(3):
        c = rng.uniform(-2.0, 2.0, N_c)
        assert np.array_equal(ccn.apply(c, N_s), rn.offsets(c, N_s)[0])
    assert (B >= 0.0).all()
    for i in range(N_s):
        first, w = ccn.row(i, N_s, N_c)
        cols = [(first + m) % N_c for m in range(4)]
        assert len(set(cols)) == 4 and np.array_equal(B[i, cols], w) and np.count_nonzero(B[i]) == np.count_nonzero(w)
        assert abs(((w[0] + w[1]) + w[2]) + w[3] - 1.0) <= 2 * np.finfo(np.float64).eps, (i, w)
        j, u = rn.basis(i, N_s, N_c)
        assert first == (j - 1) % N_c and np.array_equal(w, rn.weights(u))


HOST_MAIN = r"""
// Stand-alone host program around rl_offset_row of csrc/raceline.h.  Input: pairs [Ns, Nc] of doubles; output per pair and cell the first
// column and the four weights (5 Ns doubles).  Every buffer has its exact size on the heap, so the sanitizers see any step outside.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "raceline.h"
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb"); FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double h[2]; int cases = 0;
  while (fread(h, sizeof(double), 2, in) == 2) {
    const int Ns = (int)h[0], Nc = (int)h[1];
    std::vector<double> o((size_t)5 * Ns);
    for (int i = 0; i < Ns; ++i) {
      int col0 = -1;
      std::vector<double> w(4);
      rl_offset_row(i, Ns, Nc, col0, w.data());
      if (col0 < 0 || col0 >= Nc) abort();
      o[(size_t)5 * i] = (double)col0;
      for (int m = 0; m < 4; ++m) o[(size_t)5 * i + 1 + m] = w[m];
    }
    fwrite(o.data(), sizeof(double), o.size(), out);
    ++cases;
  }
  fclose(in); fclose(out);
  printf("built %d\n", cases);
  return 0;
}
"""


def test_host_rows_match_the_restatement_under_sanitizers(tmp_path):
    """rl_offset_row on the host, compiled with -fsanitize=address,undefined and without FMA contraction: the first column and the four
    weights of every cell, bit for bit."""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed for the host build"
    shapes = ROW_SHAPES + [(392, 196), (2048, 8)]
    np.array(shapes, dtype=np.float64).tofile(tmp_path / "in.bin")
    (tmp_path / "rows_main.cpp").write_text(HOST_MAIN)
    exe = tmp_path / "rows_main"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",   # (the runtimes inside the program: nothing to preload)
                           "-I", os.path.join(ROOT, "fsae-mpc_amd", "csrc"), str(tmp_path / "rows_main.cpp"), "-o", str(exe)])
    run = subprocess.run(["timeout", "-k", "2", "20", str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.strip() == "built %d" % len(shapes), (run.returncode, run.stdout, run.stderr)
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float64)
    off = 0
    for N_s, N_c in shapes:
        o = got[off: off + 5 * N_s].reshape(N_s, 5); off += 5 * N_s
        for i in range(N_s):
            first, w = ccn.row(i, N_s, N_c)
            assert o[i, 0] == first and np.array_equal(o[i, 1:], w), (N_s, N_c, i)
    assert off == got.size


@pytest.mark.parametrize("N_s,N_c", list(cases.SHAPES))
def test_oracle_solves_every_shape(orc, otrack, N_s, N_c):
    """fsg2019, the kappa corridor, margin 0.25: flag 0 and a KKT certificate, the line inside the corridor at every cell."""
    s = cases.oracle_cells(orc, otrack, N_s, N_c, "kappa")
    assert s["flag"] == 0, (s["flag"], s["iter"])
    free = np.full((1, N_c), ccn.FREE)
    cert = kkt_certificate(s["H"][None], s["g"][None], np.ascontiguousarray(s["B"].T)[None], -free, free, s["lbA"][None], s["ubA"][None],
                           s["x"][None], s["lam"][None])
    print("(%d, %d) %s: %d iterations, certificate %.2e, f %.5f, max |n| %.3f, max |c| %.3f, polished %d"
          % (N_s, N_c, cases.SHAPES[(N_s, N_c)], s["iter"], cert["max"][0], s["fval"], np.abs(s["n"]).max(), np.abs(s["x"]).max(), s["polished"]))
    assert cert["max"][0] <= KKT_TOL, cert
    assert abs(s["fval"] - ccn.objective(s["H"], s["g"], s["x"])) <= 1e-9 * max(1.0, abs(s["fval"]))
    assert (s["n"] >= s["lbA"] - 1e-9).all() and (s["n"] <= s["ubA"] + 1e-9).all()


def test_oracle_cell_rows_beat_the_point_boxes(orc, otrack):
    """(64, 16), what test 3 of the GPU file asserts: in the kappa corridor a cell leaves +-0.5 and the objective falls by more than
    1e-3 relative; in the constant band every cell is inside +-0.5 and the objective does not rise."""
    N_s, N_c = 64, 16
    cells, points = cases.oracle_cells(orc, otrack, N_s, N_c, "kappa"), cases.oracle_points(orc, otrack, N_s, N_c, "kappa")
    assert cells["flag"] == 0 and points["flag"] == 0
    print("kappa corridor: f %.5f (points) %.5f (cells), max |n| %.3f (points) %.3f (cells)"
          % (points["fval"], cells["fval"], np.abs(points["n"]).max(), np.abs(cells["n"]).max()))
    assert np.abs(points["n"]).max() <= cases.N_MAX - cases.MARGIN + 1e-9
    assert np.abs(cells["n"]).max() > cases.N_MAX - cases.MARGIN
    assert cells["fval"] < points["fval"] - 1e-3 * abs(points["fval"])
    cells_c, points_c = cases.oracle_cells(orc, otrack, N_s, N_c, "constant"), cases.oracle_points(orc, otrack, N_s, N_c, "constant")
    assert cells_c["flag"] == 0 and points_c["flag"] == 0
    print("constant band: f %.5f (points) %.5f (cells)" % (points_c["fval"], cells_c["fval"]))
    assert np.abs(cells_c["n"]).max() <= cases.N_MAX - cases.MARGIN + 1e-9
    assert cells_c["fval"] <= points_c["fval"]


@pytest.mark.parametrize("N_s,N_c", cases.BLOCKED_CPU)
def test_oracle_solves_a_blocked_side(orc, otrack, N_s, N_c):
    """n_lo = 0.1 over a stretch: the centre line is outside the corridor there, the QP is solved all the same."""
    assert set(cases.BLOCKED_GPU) <= set(cases.BLOCKED_CPU)
    s = cases.oracle_cells(orc, otrack, N_s, N_c, "blocked")
    assert s["flag"] == 0, (s["flag"], s["iter"])
    stretch = cases.blocked_cells(N_s)
    assert np.array_equal(s["lbA"][stretch], np.full(max(1, N_s // 10), 0.1 + cases.MARGIN))
    assert (s["n"][stretch] >= 0.35 - 1e-9).all(), s["n"][stretch]
    assert (s["n"] >= s["lbA"] - 1e-9).all() and (s["n"] <= s["ubA"] + 1e-9).all()


def test_a_pinched_cell_makes_both_bounds_nan():
    lo, hi = np.full(32, -0.75), np.full(32, 0.75)
    hi[7] = -0.75 + 2 * cases.MARGIN            # no room left in cell 7; the cells next to it interpolate towards it but keep some
    l, h = ccn.row_bounds(lo, hi, 1.0, 32.0, 32, cases.MARGIN)
    assert np.isnan(l[7]) and np.isnan(h[7]) and np.isfinite(np.delete(l, 7)).all() and np.isfinite(np.delete(h, 7)).all()
    l, h = ccn.row_bounds(lo, hi, 1.0, 32.0, 64, cases.MARGIN)       # (cells 13 and 15 of 64 lie half way: 0.5 m of room)
    assert np.isnan(l[14]) and np.isfinite(l[13]) and h[13] - l[13] == pytest.approx(0.5)


def test_new_symbols_are_declared_and_exported():
    import fsae_mpc_amd as fm
    L = fm.lib()
    header = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    for s in NEW:
        assert s in fm._lib.EXPORTS and hasattr(L, s) and ("%s(" % s) in header, s
    assert hasattr(fm.Corridor, "line_rows")


def test_rows_cells_needs_a_corridor_before_the_library_is_touched():
    code = """
import sys
sys.path.insert(0, %r)
import fsae_mpc_amd as fm
for kw, word in ((dict(rows="cells"), "Corridor.constant"), (dict(rows="cell"), "rows"), (dict(want_row_lambda=True), "rows")):
    try:
        fm.Plan.raceline(fm.KINEMATIC, None, **kw)
    except ValueError as e:
        assert word in str(e), (kw, str(e))
    else:
        raise SystemExit("no ValueError for %%r" %% (kw,))
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_cells_entries_check_their_arguments_and_compute_nothing_without_a_gpu():
    """Every refusal with its code and the full text of fsaempc_last_error; the buffers (host memory filled with a sentinel) stay as they
    were.  The texts are those of the _c entries for the same mistakes."""
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    tr = fm.Track.load("fsg2019")
    SENT = 7.0
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    xP, yP = np.ascontiguousarray(tr.xP.T, dtype=np.float64), np.ascontiguousarray(tr.yP.T, dtype=np.float64)
    sp = fm._lib.Spline(tr.M, tr.dl, p(xP), p(yP))
    N_s, N_c, P = 64, 16, 2
    tab = np.concatenate([np.full(8, -1.0), np.full(8, 1.0)])
    good = fm._lib.CorridorTable(C.c_void_p(tab.ctypes.data), C.c_void_p(tab.ctypes.data + 64), 4, tr.L / 4, 0)
    need = L.fsaempc_plan_raceline_cells_workspace_bytes(P, N_s, N_c)
    assert need > (N_c * N_c + N_s * N_c + 3 * P * N_c + 2 * P * N_s + P * (N_c + N_s)) * 8
    for args in ((0, N_s, N_c), (1, N_s, 7), (1, 500, 197), (1, 2 * N_c - 1, N_c), (1, 2049, 100)):
        assert L.fsaempc_plan_raceline_cells_workspace_bytes(*args) == -1, args
    buf = dict(line=np.full(P * N_c, SENT), table=np.full(P * N_s * 8, SENT), t=np.full(P * N_s, SENT), row_lambda=np.full(P * N_s, SENT),
               ws=np.full(need // 8 + 1, SENT), A=np.full(N_s * N_c, SENT), lbA=np.full(P * N_s, SENT), ubA=np.full(P * N_s, SENT))
    flag = np.full(P, 7, dtype=np.int32)
    blocks = np.repeat(np.asarray(fm.default_params(fm.DYNAMIC), dtype=np.float64)[None], P, axis=0).copy()
    shared, per = fm._lib.LtvParams(p(blocks), 0), fm._lib.LtvParams(p(blocks), 1)
    nan, inf = float("nan"), float("inf")

    def race(model=1, L_=tr.L, par=None, cor=good, n=1, ns=N_s, nc=N_c, m=0.25, v=20.0, gr=1.0, wsb=need, sp_=sp, line="line", lam="row_lambda"):
        return L.fsaempc_plan_raceline_cells_batch_device(model, None if sp_ is None else C.byref(sp_), C.c_double(L_), par, None if cor is None else C.byref(cor),
                                                          n, ns, nc, C.c_double(m), C.c_double(v), C.c_double(gr), None, p(buf.get(line)), p(flag),
                                                          p(buf["table"]), p(buf["t"]), p(buf.get(lam)), p(buf["ws"]), C.c_longlong(wsb), None)

    def rows(L_=tr.L, cor=good, n=1, ns=N_s, nc=N_c, m=0.25, A="A"):
        return L.fsaempc_corridor_line_rows_device(None if cor is None else C.byref(cor), C.c_double(L_), n, ns, nc, C.c_double(m), p(buf.get(A)),
                                                   p(buf["lbA"]), p(buf["ubA"]), None)

    def refused(call, code, text, **kw):
        assert call(**kw) == code, (call.__name__, kw, L.fsaempc_last_error().decode())
        assert L.fsaempc_last_error().decode() == text, (call.__name__, kw, L.fsaempc_last_error().decode())

    T = fm._lib.CorridorTable
    lo_, hi_ = C.c_void_p(tab.ctypes.data), C.c_void_p(tab.ctypes.data + 64)
    for call in (race, rows):
        refused(call, -1, "null argument (corridor)", cor=None)
        refused(call, -1, "corridor: n_lo is NULL", cor=T(None, hi_, 4, 1.0, 0))
        refused(call, -1, "corridor: n_hi is NULL", cor=T(lo_, None, 4, 1.0, 0))
        refused(call, -1, "corridor: N_w must be >= 2", cor=T(lo_, hi_, 1, 1.0, 0))
        for ds in (0.0, -1.0, nan, inf):
            refused(call, -1, "corridor: ds must be finite and > 0", cor=T(lo_, hi_, 4, ds, 0))
        for L_ in (0.0, nan, inf):
            refused(call, -1, "L must be finite and > 0", L_=L_)
        for nc, ns in ((7, N_s), (197, 500)):
            refused(call, -1, "N_c must be FSAEMPC_LINE_MIN_NC .. FSAEMPC_MAX_NV", nc=nc, ns=ns)
        for nc, ns in ((N_c, 2 * N_c - 1), (100, 2049)):
            refused(call, -1, "N_s must be 2 N_c .. FSAEMPC_LINE_MAX_NS", nc=nc, ns=ns)
        for n in (0, -3):
            refused(call, -1, "n_plans must be >= 1", n=n)
        for m in (-0.01, nan, inf, -inf):
            refused(call, -1, "margin must be finite and >= 0", m=m)
    refused(rows, -1, "null argument", A=None)
    refused(race, -1, "null argument", line=None)
    refused(race, -1, "null argument", sp_=None)
    refused(race, -1, "unknown model", model=2)
    for kw in (dict(v=0.0), dict(v=inf), dict(v=nan), dict(gr=0.0), dict(gr=nan)):
        refused(race, -1, "v_cap and grip must be finite and > 0", **kw)
    refused(race, -1, "grip must be <= 1", gr=1.5)
    refused(race, -1, "a shared parameter block makes one plan", par=C.byref(shared), n=2)
    refused(race, -5, "workspace too small", n=P, par=C.byref(per), wsb=need - 64)                 # FSAEMPC_ERR_WORKSPACE
    untouched = lambda: all(bool((a == SENT).all()) for a in buf.values()) and bool((flag == 7).all())
    assert untouched()
    if torch.cuda.is_available():
        return     # the rest states what happens without a device
    assert race() == -4 and race(lam=None) == -4 and race(n=P, par=C.byref(per)) == -4 and rows() == -4 and rows(n=P) == -4      # FSAEMPC_ERR_NODEVICE
    assert untouched()
