"""CPU tests of the lap report: the numpy restatement against a hand-made history with literal slots, the host summary
fsaempc_cl_report against the restatement's, the header's slot macros against the Python tables, the device entry's argument refusals,
and the cars of the GPU tests vetted on the oracle's closed loop (every accumulator is exercised).  The hand-made history, the rear-force
check and the oracle vetting test the restatement and the inputs -- the reference the GPU tests compare with -- not the product; the
summary, header, refusal and option tests run the product's own code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lap_numpy as ln

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT = 0.05


def _hand_history():
    """One kinematic car, six steps: outside the track on step 2 and on the finishing step 5, slack in use on step 2 (1e-9 on step 3 is
    round-off), an abnormal exit on step 3, s >= L seen on step 5.  y_d = theta_d = 0 throughout, so Fcr = 0 and e = (a / 10)^2."""
    T = 6
    h = dict(x0=np.zeros((T, 1, 5)), finished=np.zeros((T, 1), dtype=int), flag=np.zeros((T, 1), dtype=int), iter=np.zeros((T, 1), dtype=int),
             fval=np.zeros((T, 1)), slack=np.zeros((T, 1, 1)), a=np.zeros((T, 1)), cart=np.zeros((T, 1, 7)))
    h["x0"][:, 0, 0] = [1, 2, 3, 4, 5, 6]
    h["x0"][:, 0, 1] = [0.1, 0.5, -0.95, 0.5, 0.25, 0.85]
    h["finished"][:, 0] = [0, 0, 0, 0, 0, 1]
    h["flag"][:, 0] = [0, 0, 0, -2, 0, 0]
    h["iter"][:, 0] = [7, 9, 12, 100, 8, 55]
    h["fval"][:, 0] = [10, 20, 30, np.nan, 40, 1e9]
    h["slack"][:, 0, 0] = [0, 0, 0.03, 1e-9, 0, 0.5]
    h["a"][:, 0] = [5, 12, 10, 0, -11, 30]
    h["cart"][:, 0, 3] = [3, 4, 5, 6, 7, 8]
    return h


def test_restatement_on_a_hand_made_history():
    r = ln.car_record(_hand_history(), 0, DT, 1e-6)
    want = {"STEPS": 5, "STATUS": 1, "N_VIOL_INT": 0.015, "N_VIOL_MAX": 0.2, "N_ABS_MAX": 0.95, "ABNORMAL": 1, "OBJ_SUM": 70.0, "OBJ_CNT": 3,
            "SLACK_N_CNT": 1, "SLACK_TYRE_CNT": 1, "ELL_VIOL_INT": 0.0325, "ELL_VIOL_MAX": 0.44, "ITER_SUM": 136, "ITER_MAX": 100,
            "S_START": 1.0, "S_LAST": 5.0}
    assert set(want) == set(ln.SLOTS)
    for name, v in want.items():
        assert abs(r[ln.IDX[name]] - v) <= 1e-13, (name, r[ln.IDX[name]], v)
    # the threshold: with slack_tol = 0 the round-off slack of step 3 counts as in use; a lost car only latches
    assert ln.car_record(_hand_history(), 0, DT, 0.0)[ln.IDX["SLACK_N_CNT"]] == 2
    h = _hand_history(); h["finished"][2:, 0] = 2
    r = ln.car_record(h, 0, DT, 1e-6)
    assert r[ln.IDX["STATUS"]] == 2 and r[ln.IDX["STEPS"]] == 2 and r[ln.IDX["N_ABS_MAX"]] == 0.5 and r[ln.IDX["S_LAST"]] == 2.0
    # a NaN slack is not in use
    h = _hand_history(); h["slack"][0, 0, 0] = np.nan
    assert ln.car_record(h, 0, DT, 1e-6)[ln.IDX["SLACK_N_CNT"]] == 1


def test_restated_rear_force_is_the_oracles(orc, otrack):
    rng = np.random.default_rng(5)
    c = ln.constants(None)
    for _ in range(32):
        x = np.concatenate([[rng.uniform(0, 100), rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.2), rng.uniform(0, 25)], rng.uniform(-1, 1, 3)])
        f, F = np.zeros(7), C.c_double(0)
        orc.lib().orc_f_dyn(x.ctypes.data_as(C.POINTER(C.c_double)), np.zeros(2).ctypes.data_as(C.POINTER(C.c_double)), C.byref(otrack.c),
                            f.ctypes.data_as(C.POINTER(C.c_double)), C.byref(F))
        assert abs(ln.fcr(c, x) - F.value) <= 1e-12 * max(1.0, abs(F.value))


def _random_records(rng, B, status):
    rec = np.zeros((B, 16))
    I = ln.IDX
    rec[:, I["STEPS"]] = rng.integers(0, 400, B)
    rec[:, I["STATUS"]] = status
    for name in ("ABNORMAL", "OBJ_CNT", "SLACK_N_CNT", "SLACK_TYRE_CNT"):
        rec[:, I[name]] = np.floor(rec[:, I["STEPS"]] * rng.uniform(0, 1, B))
    rec[:, I["OBJ_SUM"]] = rec[:, I["OBJ_CNT"]] * rng.uniform(100, 1e4, B)
    for name in ("N_VIOL_INT", "N_VIOL_MAX", "N_ABS_MAX", "ELL_VIOL_INT", "ELL_VIOL_MAX"):
        rec[:, I[name]] = rng.uniform(0, 2, B) * (rng.uniform(0, 1, B) > 0.4)
    rec[:, I["ITER_MAX"]] = rng.integers(0, 100, B)
    rec[:, I["ITER_SUM"]] = rec[:, I["STEPS"]] * rng.integers(5, 30, B)
    rec[:, I["S_START"]] = rng.uniform(0, 300, B); rec[:, I["S_LAST"]] = rng.uniform(0, 300, B)
    return rec


def _report(fm, rec, dt):
    rec = np.ascontiguousarray(rec, dtype=np.float64)
    out = np.full(fm.NREPORT, -777.0)
    rc = fm.lib().fsaempc_cl_report(C.c_void_p(rec.ctypes.data) if rec.size else None, rec.shape[0], C.c_double(dt), C.c_void_p(out.ctypes.data))
    return rc, out


@pytest.mark.parametrize("case", ["mixed 37", "batch 1 finished", "batch 1 driving", "all lost", "none finished", "no steps", "empty"])
def test_host_summary_is_the_restatements(case):
    import fsae_mpc_amd as fm
    rng = np.random.default_rng(11)
    if case == "mixed 37":
        rec = _random_records(rng, 37, rng.integers(0, 3, 37))
    elif case == "batch 1 finished":
        rec = _random_records(rng, 1, 1); rec[0, 0] = 321
    elif case == "batch 1 driving":
        rec = _random_records(rng, 1, 0)
    elif case == "all lost":
        rec = np.zeros((9, 16)); rec[:, 1] = 2
    elif case == "none finished":
        rec = _random_records(rng, 12, rng.integers(0, 2, 12) * 2)
    elif case == "no steps":
        rec = np.zeros((4, 16))
    else:
        rec = np.zeros((0, 16))
    rc, out = _report(fm, rec, DT)
    assert rc == 0
    want = ln.summary(rec, DT)
    assert list(fm.REPORT_INDEX) == ln.SUMMARY
    for name, i in fm.REPORT_INDEX.items():
        w = want[name]
        if np.isnan(w):
            assert np.isnan(out[i]), (name, out[i])
        else:
            assert abs(out[i] - w) <= 1e-12 * max(1.0, abs(w)), (name, out[i], w)
    nan_means = {"all lost": ["LAP_MEAN", "LAP_MIN", "LAP_MAX", "ABNORMAL_PCT", "SLACK_N_PCT", "OBJ_MEAN", "N_VIOL_INT_MEAN", "ITER_MEAN"],
                 "none finished": ["LAP_MEAN", "LAP_MIN", "LAP_MAX"], "batch 1 driving": ["LAP_MEAN"]}.get(case, [])
    for name in nan_means:
        assert np.isnan(out[fm.REPORT_INDEX[name]]), name
    if case == "batch 1 finished":
        assert out[fm.REPORT_INDEX["LAP_MEAN"]] == 321 * DT == out[fm.REPORT_INDEX["LAP_MIN"]] == out[fm.REPORT_INDEX["LAP_MAX"]]
    if case == "all lost":
        assert out[fm.REPORT_INDEX["CARS_LOST"]] == 9 and out[fm.REPORT_INDEX["CARS_FINISHED"]] == 0
    rc2, out2 = _report(fm, rec, DT)
    assert np.array_equal(out, out2, equal_nan=True)            # fixed order: the same bits
    # the summary's own refusals
    assert _report(fm, rec, 0.0)[0] == -1 and _report(fm, rec, float("nan"))[0] == -1 and _report(fm, rec, float("inf"))[0] == -1
    assert fm.lib().fsaempc_cl_report(C.c_void_p(rec.ctypes.data) if rec.size else None, -1, C.c_double(DT), C.c_void_p(out.ctypes.data)) == -1
    assert fm.lib().fsaempc_cl_report(None, 3, C.c_double(DT), C.c_void_p(out.ctypes.data)) == -1
    assert fm.lib().fsaempc_cl_report(C.c_void_p(out.ctypes.data), 1, C.c_double(DT), None) == -1


def test_lap_report_object_on_host_records():
    import fsae_mpc_amd as fm
    rec = _random_records(np.random.default_rng(3), 6, np.array([0, 1, 1, 2, 0, 1]))
    rep = fm.LapReport(rec, DT)
    assert np.array_equal(rep.steps, rec[:, 0]) and np.array_equal(rep.status, rec[:, 1]) and np.array_equal(rep.s_last, rec[:, 15])
    assert np.array_equal(rep.lap_time, rec[:, 0] * DT)
    s, want = rep.summary(), ln.summary(rec, DT)
    assert set(s) == {k.lower() for k in ln.SUMMARY} and s["cars_finished"] == 3.0
    assert all(abs(s[k.lower()] - want[k]) <= 1e-12 * max(1.0, abs(want[k])) for k in ln.SUMMARY)


def test_header_slots_match_the_python_tables():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FSAEMPC_M_([A-Z_0-9]+)\s+(\d+)", hdr)}
    assert slots == fm.METRIC_INDEX and list(fm.METRIC_INDEX) == ln.SLOTS
    assert int(re.search(r"#define\s+FSAEMPC_NMETRIC\s+(\d+)", hdr).group(1)) == fm.NMETRIC == len(slots) == 16
    assert sorted(slots.values()) == list(range(16))
    rows = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FSAEMPC_R_([A-Z_0-9]+)\s+(\d+)", hdr)}
    assert rows == fm.REPORT_INDEX and int(re.search(r"#define\s+FSAEMPC_NREPORT\s+(\d+)", hdr).group(1)) == fm.NREPORT == len(rows)
    for s in ("fsaempc_cl_metrics_batch_device", "fsaempc_cl_report"):
        assert s in fm._lib.EXPORTS and hasattr(fm.lib(), s) and ("int %s(" % s) in hdr, s
    for name in ("LapReport", "METRIC_INDEX", "NMETRIC", "REPORT_INDEX", "NREPORT"):
        assert name in fm.__all__ and hasattr(fm, name)


def test_metrics_entry_refuses_bad_arguments_before_any_launch():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    B, N = 3, 10
    p = lambda a: C.c_void_p(a.data_ptr())
    nan, inf = float("nan"), float("inf")
    for model in (fm.KINEMATIC, fm.DYNAMIC):
        nx, ns = fm.dims(model, N)[:2]
        f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64)
        i32 = lambda *s: torch.full(s, 7, dtype=torch.int32)
        bufs = dict(x0=f64(B, nx), finished=i32(B), exitflag=i32(B), iter=i32(B), fval=f64(B), slack=f64(B, ns), u=f64(B, 2 * N), cart=f64(B, 7),
                    metrics=f64(B, 16))
        order = ["x0", "finished", "exitflag", "iter", "fval", "slack", "u", "cart", "metrics"]
        blocks = torch.from_numpy(np.repeat(fm.default_params(model)[None], B, axis=0).copy())

        def call(model_=model, N_=N, dt=DT, tol=1e-6, batch=B, par=None, null=None):
            return L.fsaempc_cl_metrics_batch_device(model_, N_, C.c_double(dt), C.c_double(tol), batch, par,
                                                     *[None if k == null else p(bufs[k]) for k in order], None)
        for k in order:
            assert call(null=k) == -1, k
        for kw in (dict(model_=2), dict(model_=-1), dict(N_=0), dict(dt=0.0), dict(dt=-DT), dict(dt=nan), dict(dt=inf), dict(tol=-1e-9), dict(tol=nan),
                   dict(batch=-1)):
            assert call(**kw) == -1, kw
        assert call(tol=-1.0) == -1 and b"slack_tol" in L.fsaempc_last_error()
        assert call(batch=0) == 0                                     # nothing to launch: succeeds on any machine
        shared, per = fm._lib.LtvParams(p(blocks), 0), fm._lib.LtvParams(p(blocks), 1)
        assert call(batch=0, par=C.byref(shared)) == 0 and call(batch=0, par=C.byref(per)) == 0
        assert all(bool((bufs[k] == 7).all()) for k in order)
        if torch.cuda.is_available():
            continue     # the rest states what happens without a device
        assert call() == -4 and call(par=C.byref(shared)) == -4 and call(par=C.byref(per)) == -4    # FSAEMPC_ERR_NODEVICE: no CPU path
        assert all(bool((bufs[k] == 7).all()) for k in order)


def test_python_options_are_checked_before_the_library_is_touched():
    import subprocess, sys
    code = """
import sys
sys.path.insert(0, %r)
import fsae_mpc_amd as fm
for tol in (-1e-9, float("nan")):
    try:
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, [[0.0] * 7], metrics=True, slack_tol=tol)
    except ValueError:
        continue
    raise SystemExit("no ValueError for slack_tol = %%r" %% tol)
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_inputs_vetted_on_the_oracle(orc, otrack):
    """The cars of GPU test A on the oracle's closed loop (kinematic, N = 10, fsg2019, 30 steps): every accumulator is exercised, and the
    slack threshold is not in play (no slack value between 1e-9 and 1e-4)."""
    cart, s0, v0, kind = ln.cars(otrack, 5)
    h = ln.drive_oracle(orc, otrack, 0, 10, DT, cart, s0, v0, 30)
    r = ln.records(h, DT, 1e-6)
    I = ln.IDX
    centre, off, end, lost, mirror = r
    assert centre[I["STATUS"]] == 0 and centre[I["STEPS"]] == 30 and centre[I["N_VIOL_INT"]] == 0 and centre[I["SLACK_N_CNT"]] == 0
    assert (h["slack"][:, 0, 0] == 0).all() and centre[I["OBJ_CNT"]] == 30 and centre[I["OBJ_SUM"]] > 0
    assert (np.abs(h["x0"][:, 1, 1]) > 0.75).sum() == 9 and off[I["N_VIOL_INT"]] > 0 and abs(off[I["N_VIOL_MAX"]] - 0.15) < 1e-6
    sl = h["slack"][:, 1, 0]
    assert (sl > 1e-6).sum() == 8 == off[I["SLACK_N_CNT"]] == off[I["SLACK_TYRE_CNT"]] and abs(sl.max() - 0.148) < 1e-3
    assert not ((h["slack"] > 1e-9) & (h["slack"] < 1e-4)).any()
    assert off[I["STATUS"]] == 0 and off[I["OBJ_CNT"]] == 22 and off[I["ITER_SUM"]] > 0 and off[I["ITER_MAX"]] > 0
    assert end[I["STATUS"]] == 1 and end[I["STEPS"]] == 5 and abs(h["x0"][5, 2, 0] - otrack.L - 0.067) < 1e-3
    assert end[I["S_START"]] == h["x0"][0, 2, 0] and end[I["S_LAST"]] == h["x0"][4, 2, 0] and end[I["N_ABS_MAX"]] == np.abs(h["x0"][:6, 2, 1]).max()
    assert lost[I["STATUS"]] == 2 and lost[I["STEPS"]] == 0 and np.count_nonzero(lost) == 1
    assert mirror[I["N_VIOL_INT"]] > 0 and mirror[I["STATUS"]] == 0
    # default axes: the off-line car's ellipse value peaks at 1.083; with ELL_LONG = 1, ELL_LAT = 2 it exceeds 1 on 19 of 30 steps
    c = ln.constants(None)
    e = np.array([ln.ellipse(c, h["cart"][t, 1], h["a"][t, 1]) for t in range(30)])
    assert abs(e.max() - 1.083) < 1e-3 and off[I["ELL_VIOL_INT"]] > 0
    import fsae_mpc_amd as fm
    P = fm.default_params(fm.KINEMATIC); P[fm.PARAM_INDEX["ELL_LONG"]] = 1.0; P[fm.PARAM_INDEX["ELL_LAT"]] = 2.0
    c2 = ln.constants(P)
    assert c2["ELL_LONG"] == 1.0 and c2["ELL_LAT"] == 2.0 and c2["N_MAX"] == 0.75 and c2["M"] == 280.0
    e2 = np.array([ln.ellipse(c2, h["cart"][t, 1], h["a"][t, 1]) for t in range(30)])
    r2 = ln.records(h, DT, 1e-6, P)
    assert (e2 > 1).sum() == 19 and r2[1, I["ELL_VIOL_INT"]] > 0 and r2[1, I["ELL_VIOL_MAX"]] > 1
    # no abnormal exit among these cars: that accumulator is exercised by the hand-made history
    assert (h["flag"] == 0).all()
    # the restated block positions are the product's table
    assert all(fm.PARAM_INDEX[k] == i for k, i in ln.BLOCK_POS.items())
