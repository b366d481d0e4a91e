"""CPU tests of the s-varying track corridors: the numpy restatement (tests/corridor_numpy.py) against hand-made
literals and a brute-force loop, the C ABI of the new entries against include/fsaempc.h, and what Python refuses before the library
is touched."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import corridor_numpy as cn

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_lookup_against_literals():
    t = np.array([1.0, 2.0, 4.0, 8.0])     # 4 cells of 2 m: L = 8
    ds = 2.0
    assert cn.lookup(t, ds, 0.0) == 1.0                      # s = 0
    assert cn.lookup(t, ds, 4.0) == 4.0                      # exactly on a cell
    assert cn.lookup(t, ds, 5.0) == 6.0                      # mid-cell: 4 + 0.5 (8 - 4)
    assert cn.lookup(t, ds, 7.0) == 4.5                      # the last cell wraps to cell 0: 8 + 0.5 (1 - 8)
    assert cn.lookup(t, ds, 7.5) == 2.75
    assert cn.lookup(t, ds, -1.0) == 4.5                     # s < 0: the same point as s = 7
    assert cn.lookup(t, ds, -8.0) == 1.0 and cn.lookup(t, ds, -3.0) == 6.0
    assert cn.lookup(t, ds, 9.0) == 1.5                      # s > L: the same point as s = 1
    assert cn.lookup(t, ds, 8.0) == 1.0 and cn.lookup(t, ds, 21.0) == 6.0
    assert np.array_equal(cn.lookup(t, ds, np.array([[0.0, 5.0], [9.0, -1.0]])), [[1.0, 6.0], [1.5, 4.5]])
    assert np.isnan(cn.lookup(t, ds, np.nan)) and np.isnan(cn.lookup(t, ds, np.inf))


def test_constant_table_returns_the_constant_exactly():
    rng = np.random.default_rng(5)
    s = np.concatenate([rng.uniform(-700.0, 900.0, 4000), [0.0, 311.0, -1e-20, 1e-300]])
    for c in (0.75, -0.75, 0.1, 1.0 / 3.0):
        for Nw in (2, 7, 200):
            assert np.array_equal(cn.lookup(np.full(Nw, c), 311.0 / Nw, s), np.full(s.size, c))


def test_limits_are_nan_only_where_a_cell_read_is_invalid():
    lo = np.array([-1.0, -1.0, 0.5, -1.0])
    hi = np.array([1.0, 1.0, 0.5, 1.0])          # cell 2: n_lo < n_hi does not hold
    s = np.array([0.5, 2.5, 4.5, 6.5, 2.0, np.nan])
    l, h = cn.limits(lo, hi, 2.0, s)
    assert np.array_equal(np.isnan(l), [False, True, True, False, True, True]) and np.array_equal(np.isnan(l), np.isnan(h))
    assert l[0] == -1.0 and h[3] == 1.0
    lb, ub = cn.row_bounds(lo, hi, 2.0, np.array([0.5, 6.5]), np.array([0.25, -0.25]))
    assert np.array_equal(lb, [-1.25, -0.75]) and np.array_equal(ub, [0.75, 1.25])
    assert np.array_equal(cn.violation(lo, hi, 2.0, np.array([0.5, 0.5, 0.5, 2.5]), np.array([1.5, -1.25, 0.5, 3.0])), [0.5, 0.25, 0.0, 0.0])


def test_control_point_bounds_against_a_brute_force_loop():
    """N_s = 64, N_c = 16.  The loop goes the other way round: every cell hands its limits to the four control points its basis weights
    (first control point floor(i N_c / N_s) - 1)."""
    N_s, N_c, L, margin, Nw = 64, 16, 311.0, 0.25, 50
    s_w = np.arange(Nw) * L / Nw
    n_hi = 0.75 + 0.75 * np.sin(3 * np.pi * s_w / L) ** 2
    n_lo = -(0.75 + 0.5 * np.sin(2 * np.pi * s_w / L + 0.7) ** 2)
    n_hi[(s_w > 100) & (s_w < 115)] = 0.6
    lb, ub = cn.control_point_bounds(n_lo, n_hi, L / Nw, L, N_s, N_c, margin)
    wl, wu = np.full(N_c, -np.inf), np.full(N_c, np.inf)
    for i in range(N_s):
        s = i * L / N_s
        q = s / (L / Nw)
        k = int(np.floor(q)) % Nw
        u = q - np.floor(q)
        lo = n_lo[k] + u * (n_lo[(k + 1) % Nw] - n_lo[k])
        hi = n_hi[k] + u * (n_hi[(k + 1) % Nw] - n_hi[k])
        j0 = (i * N_c) // N_s
        for m in range(4):
            j = (j0 - 1 + m) % N_c
            wl[j] = max(wl[j], lo + margin)
            wu[j] = min(wu[j], hi - margin)
    assert np.abs(lb - wl).max() <= 1e-14 and np.abs(ub - wu).max() <= 1e-14
    assert [cn.touching_cells(j, N_s, N_c).size for j in range(N_c)] == [16] * N_c
    assert np.array_equal(cn.touching_cells(0, N_s, N_c), list(range(0, 8)) + list(range(56, 64)))
    # a cell that is not valid voids exactly the control points it touches
    bad_hi = n_hi.copy(); bad_hi[10] = n_lo[10]
    lb2, ub2 = cn.control_point_bounds(n_lo, bad_hi, L / Nw, L, N_s, N_c, margin)
    touched = np.zeros(N_c, dtype=bool)
    for i in range(N_s):
        k = int(np.floor(i * L / N_s / (L / Nw)))
        if k in (9, 10):
            touched[[((i * N_c) // N_s - 1 + m) % N_c for m in range(4)]] = True
    assert np.array_equal(np.isnan(lb2), touched) and np.array_equal(np.isnan(ub2), touched) and touched.any() and not touched.all()


def test_struct_layout_and_prototypes_match_the_header(tmp_path):
    """fsaempc_corridor as the C compiler lays it out against the ctypes mirror, and the four new prototypes: a translation unit that
    assigns each entry to a pointer of the type the binding assumes compiles without a diagnostic only if the header agrees."""
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text(r"""
#include <stdio.h>
#include <stddef.h>
#include "fsaempc.h"
typedef const double* cd; typedef double* d; typedef const int* ci;
int (*build_c)(const fsaempc_ltv_desc*, const fsaempc_spline*, const fsaempc_ltv_params*, const fsaempc_ltv_blocking*, const fsaempc_corridor*,
               cd, cd, cd, cd, d, d, d, d, d, d, d, d, d, d, void*) = fsaempc_ltv_build_qp_batch_device_c;
int (*step_c)(const fsaempc_ltv_desc*, const fsaempc_spline*, const fsaempc_ltv_params*, const fsaempc_ltv_blocking*, const fsaempc_corridor*,
              cd, cd, cd, cd, const fsaempc_qp_opts*, d, d, d, d, int*, int*, d, const fsaempc_qp_aux*, void*, long long, void*) = fsaempc_ltv_step_batch_device_c;
int (*metrics_c)(int, int, double, double, int, const fsaempc_ltv_params*, const fsaempc_corridor*, cd, ci, ci, ci, cd, cd, cd, cd, d, void*) = fsaempc_cl_metrics_batch_device_c;
int (*raceline_c)(int, const fsaempc_spline*, double, const fsaempc_ltv_params*, const fsaempc_corridor*, int, int, int, double, double, double,
                  const fsaempc_qp_opts*, d, int*, d, d, void*, long long, void*) = fsaempc_plan_raceline_batch_device_c;
int (*bounds_c)(const fsaempc_corridor*, double, int, int, int, double, d, d, void*) = fsaempc_corridor_line_bounds_device;
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(fsaempc_corridor), offsetof(fsaempc_corridor, n_lo), offsetof(fsaempc_corridor, n_hi),
         offsetof(fsaempc_corridor, N_w), offsetof(fsaempc_corridor, ds), offsetof(fsaempc_corridor, per_instance));
  return 0;
}
""")
    inc = os.path.join(ROOT, "include")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # (the entries are not linked: the layout line comes from a second unit without the pointers)
    src2 = tmp_path / "layout2.c"
    src2.write_text(src.read_text().split("typedef const double* cd;")[0] + "int main(void) {" + src.read_text().split("int main(void) {")[1])
    exe = tmp_path / "layout2"
    subprocess.check_call(["gcc", "-std=c11", "-I", inc, str(src2), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T = _lib.CorridorTable
    assert got == [C.sizeof(T), T.n_lo.offset, T.n_hi.offset, T.N_w.offset, T.ds.offset, T.per_instance.offset], got
    L = fm.lib()
    for name, n_args in (("fsaempc_ltv_build_qp_batch_device_c", 20), ("fsaempc_ltv_step_batch_device_c", 21),
                         ("fsaempc_cl_metrics_batch_device_c", 17), ("fsaempc_plan_raceline_batch_device_c", 19),
                         ("fsaempc_corridor_line_bounds_device", 9)):
        assert name in _lib.EXPORTS and len(getattr(L, name).argtypes) == n_args, name


def test_corridor_validation_happens_on_the_host():
    import fsae_mpc_amd as fm
    lo, hi = -np.ones(8), np.ones(8)
    with pytest.raises(ValueError, match="shapes disagree"):
        fm.Corridor.from_table(lo, np.ones(9), 100.0, device="cpu")
    with pytest.raises(ValueError, match="shapes disagree"):
        fm.Corridor.from_table(np.tile(lo, (2, 1)), hi, 100.0, device="cpu")
    for v in (1.0, 1.5):                       # n_lo == n_hi and n_lo > n_hi
        bad = lo.copy(); bad[3] = v
        with pytest.raises(ValueError, match="n_lo < n_hi"):
            fm.Corridor.from_table(bad, hi, 100.0, device="cpu")
    for v in (np.nan, np.inf, -np.inf):
        bad = hi.copy(); bad[5] = v
        with pytest.raises(ValueError, match="finite"):
            fm.Corridor.from_table(lo, bad, 100.0, device="cpu")
        with pytest.raises(ValueError, match="finite"):
            fm.Corridor.from_table(-bad, hi, 100.0, device="cpu")
    with pytest.raises(ValueError, match="N_w >= 2"):
        fm.Corridor.from_table([-1.0], [1.0], 100.0, device="cpu")
    for L in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="L must be"):
            fm.Corridor.from_table(lo, hi, L, device="cpu")
    with pytest.raises(ValueError, match="half_width"):
        fm.Corridor.constant(100.0, 0.0, device="cpu")
    with pytest.raises(ValueError, match="N_w"):
        fm.Corridor.constant(100.0, 0.75, N_w=1, device="cpu")
    c = fm.Corridor.from_table(lo, hi, 100.0, device="cpu")
    assert (c.P, c.N_w, c.ds, c.c.per_instance, c.c.N_w, c.c.ds) == (1, 8, 12.5, 0, 8, 12.5)
    c3 = fm.Corridor.from_table(np.tile(lo, (3, 1)), np.tile(hi, (3, 1)), 100.0, device="cpu")
    assert (c3.P, c3.N_w, c3.c.per_instance) == (3, 8, 1)
    k = fm.Corridor.constant(100.0, 0.75, device="cpu")
    assert k.N_w == 2 and k.ds == 50.0 and k.n_lo.tolist() == [[-0.75, -0.75]] and k.n_hi.tolist() == [[0.75, 0.75]]


def test_wrong_batch_and_device_are_refused_before_the_library():
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    c3 = fm.Corridor.from_table(-np.ones((3, 8)), np.ones((3, 8)), tr.L, device="cpu")
    c1 = fm.Corridor.constant(tr.L, 0.75, device="cpu")
    c3.check_batch(3); c1.check_batch(3); c1.check_batch(64)
    with pytest.raises(ValueError, match="holds 3 tables"):
        fm.LtvBatch(fm.KINEMATIC, 10, 0.05, tr, 4, corridor=c3)
    with pytest.raises(ValueError, match="holds 3 tables"):
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, tr, np.zeros((4, 7)), corridor=c3)
    with pytest.raises(ValueError, match="holds 3 tables"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, n_plans=2, corridor=c3)
    with pytest.raises(ValueError, match="is on cpu"):
        fm.LtvBatch(fm.KINEMATIC, 10, 0.05, tr, 3, corridor=c3)
    with pytest.raises(ValueError, match="is on cpu"):
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, tr, np.zeros((4, 7)), corridor=c1, device="cuda:0")
    with pytest.raises(ValueError, match="is on cpu"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, corridor=c3)
    with pytest.raises(ValueError, match="None or a Corridor"):
        fm.LtvBatch(fm.KINEMATIC, 10, 0.05, tr, 4, corridor=(-np.ones(8), np.ones(8)))
    with pytest.raises(ValueError, match="None or a Corridor"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, corridor=(-np.ones(8), np.ones(8)))
    # Plan.raceline's plan count: a per-plan corridor sets it only when nothing else has (no blocks, n_plans left at 1); blocks of
    # (P, 32) set it themselves and the corridor must then agree; one shared block makes one plan and cannot go with P corridors
    blocks = np.repeat(fm.default_params(fm.KINEMATIC)[None], 2, axis=0)
    with pytest.raises(ValueError, match="holds 3 tables"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, params=blocks, corridor=c3)
    with pytest.raises(ValueError, match="holds 3 tables"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, params=blocks[:1], corridor=c3)
    with pytest.raises(ValueError, match="shared parameter block makes one plan, the corridor holds 3"):
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, params=blocks[0], corridor=c3)
    with pytest.raises(ValueError, match="is on cpu"):       # (three blocks, three corridors, n_plans inferred: past the count checks)
        fm.Plan.raceline(fm.KINEMATIC, tr, N_s=64, N_c=16, params=np.repeat(blocks[:1], 3, axis=0), corridor=c3)


def test_paths_without_a_corridor_form_refuse_a_corridor_batch():
    """The exact build of the SQP, the affine maps and the VJPs have no corridor form: they refuse, as they do for move blocking."""
    import fsae_mpc_amd as fm
    tr = fm.Track.load("fsg2019")
    cor = fm.Corridor.constant(tr.L, 0.75, device="cpu")
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.SqpBatch(fm.KINEMATIC, 10, 0.05, tr, 4, corridor=cor)
    batch = types.SimpleNamespace(params=None, blocking=None, corridor=cor)    # what the refusal reads of an LtvBatch
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.ltv_step_affine_maps(batch, None, None)
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.ltv_step_lambda(batch, None, None, None, None)
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.ltv_step_vjp(batch, {}, None, None, None, None)
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.ltv_step_diff(batch, None, None, None, None)
    with pytest.raises(NotImplementedError, match="corridor"):
        fm.feedback_gain(batch, None, None, None, None)


def test_c_entries_refuse_a_bad_corridor_before_anything_else():
    """FSAEMPC_ERR_ARG with the argument named; host code only, so this runs without a GPU.  (Every other argument is NULL: a corridor
    that passed would be refused for those next, with another message.)"""
    import fsae_mpc_amd as fm
    from fsae_mpc_amd import _lib
    L = fm.lib()
    buf = (C.c_double * 4)()
    ptr = C.cast(buf, C.c_void_p)
    cases = [((None, ptr, 4, 1.0), "n_lo"), ((ptr, None, 4, 1.0), "n_hi"), ((ptr, ptr, 1, 1.0), "N_w"), ((ptr, ptr, 4, 0.0), "ds"),
             ((ptr, ptr, 4, -1.0), "ds"), ((ptr, ptr, 4, float("nan")), "ds"), ((ptr, ptr, 4, float("inf")), "ds")]
    for (lo, hi, Nw, ds), word in cases:
        cor = _lib.CorridorTable(lo, hi, Nw, ds, 0)
        calls = [lambda: L.fsaempc_ltv_build_qp_batch_device_c(None, None, None, None, C.byref(cor), *([None] * 15)),
                 lambda: L.fsaempc_ltv_step_batch_device_c(None, None, None, None, C.byref(cor), *([None] * 13), None, 0, None),
                 lambda: L.fsaempc_cl_metrics_batch_device_c(0, 10, 0.05, 1e-6, 4, None, C.byref(cor), *([None] * 10)),
                 lambda: L.fsaempc_plan_raceline_batch_device_c(0, None, 100.0, None, C.byref(cor), 1, 64, 16, 0.25, 20.0, 1.0, None,
                                                                None, None, None, None, None, 0, None),
                 lambda: L.fsaempc_corridor_line_bounds_device(C.byref(cor), 100.0, 1, 64, 16, 0.25, None, None, None)]
        for call in calls:
            assert call() == -1
            msg = L.fsaempc_last_error().decode()
            assert "corridor" in msg and word in msg, (word, msg)
