"""CPU tests of the multi-lap closed loop: the numpy restatement of the lap gate (tests/laps_numpy.py) against a hand-made
history with literal values, the host entry fsaempc_cl_lap_summary against numpy, the header's macros against the Python tables, every
refusal of the gate entry and of the Python options without a device, and the cars and tracks of the GPU tests vetted on the oracle's closed
loop with the restated gate in it.  The hand-made history and the vetting test the restatement and the inputs -- the reference the GPU
tests compare with -- not the product; the summary, header and refusal tests run the product's own code."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lap_numpy as ln
import laps_numpy as lp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DT = 0.05


def test_restatement_on_a_hand_made_history():
    """Four kinematic cars, L = 100, dt = 0.05, laps = 3, N = 2.  Car 0 crosses on calls 2 and 4 and finally on call 6; car 1 is lost from
    call 1 on; car 2 is past the line on the very first call (k = 0); car 3 is seen past the line with s == S_PREV."""
    L, laps, N, nx = 100.0, 3, 2, 5
    st, times, recs = lp.fresh(4, laps, metrics=True)
    metrics = np.zeros((4, 16))
    fin = np.zeros(4, dtype=int)
    #          car 0   car 1  car 2   car 3
    s_seen = [[96.0,   50.0,  100.5,  99.0],
              [98.0,   0.0,   1.0,    99.0],     # car 1: the pre-step's placeholder; car 3 did not move ...
              [101.0,  0.0,   2.0,    99.0],
              [3.0,    0.0,   3.0,    99.0],
              [100.5,  0.0,   4.0,    99.0],
              [2.0,    0.0,   5.0,    99.0],
              [100.25, 0.0,   6.0,    99.0]]
    seen = []
    for call, s in enumerate(s_seen):
        x0 = np.zeros((4, nx)); x0[:, 0] = s; x0[:, 1] = 0.25
        x_ref = np.zeros((4, N, nx)); x_ref[:, :, 0] = np.array(s)[:, None] + [[1.0, 2.0]]; x_ref[:, :, 3] = 7.0
        x_keep = np.zeros((4, N, nx)); x_keep[:, :, 0] = np.array(s)[:, None] + [[0.5, 1.5]]; x_keep[:, :, 2] = -3.0
        fin[(np.array(s) >= L) & (fin == 0)] = 1
        if call >= 1:
            fin[1] = 2
        if call == 3:
            fin[3] = 1                                   # ... and a pre-step flags it all the same: s == S_PREV
        metrics[:, :] = 10.0 * call + np.arange(16)[None, :] + 100.0 * np.arange(4)[:, None]
        lp.gate(DT, L, laps, x0, x_ref, x_keep, fin, st, times, metrics, recs)
        seen.append(dict(x0=x0.copy(), x_ref=x_ref.copy(), x_keep=x_keep.copy(), fin=fin.copy(), metrics=metrics.copy()))
    # car 0: crossing 1 on call 2 (k = 2, S_PREV = 98): f = 2/3, t = (1 + 2/3) dt; crossing 2 on call 4 (k = 4, S_PREV = 3): f = 97/97.5;
    # final crossing on call 6 (k = 6, S_PREV = 2): f = 98 / 98.25
    t1, t2, t3 = (1 + 2.0 / 3.0) * DT, (3 + 97.0 / 97.5) * DT, (5 + 98.0 / 98.25) * DT
    assert np.allclose(times[0], [t1, t2 - t1, t3 - t2], rtol=0, atol=1e-15)
    assert abs(times[0, 0] - 0.08333333333333333) < 1e-15 and abs(times[0, 1] - 0.11641025641025641) < 1e-15
    assert st[0, lp.DONE] == 3 and st[0, lp.STEPS] == 6 and st[0, lp.S_PREV] == 2.0 and abs(st[0, lp.T_CROSS] - t3) < 1e-15
    assert seen[2]["x0"][0, 0] == 1.0 and seen[2]["fin"][0] == 0 and np.array_equal(seen[2]["x_ref"][0, :, 0], [2.0, 3.0])
    assert np.array_equal(seen[2]["x_keep"][0, :, 0], [1.5, 2.5]) and np.array_equal(seen[2]["x_keep"][0, :, 2], [-3.0, -3.0])
    assert np.array_equal(seen[2]["x_ref"][0, :, 3], [7.0, 7.0]) and seen[2]["x0"][0, 1] == 0.25
    assert seen[4]["x0"][0, 0] == 0.5 and seen[4]["fin"][0] == 0
    assert seen[6]["x0"][0, 0] == 100.25 and seen[6]["fin"][0] == 1 and np.array_equal(seen[6]["x_ref"][0, :, 0], [101.25, 102.25])
    # records: handed over with STATUS 1 at the intermediate crossings, the live record zeroed; the final crossing touches neither
    want = 20.0 + np.arange(16); want[ln.IDX["STATUS"]] = 1.0
    assert np.array_equal(recs[0, 0], want) and not seen[2]["metrics"][0].any()
    want = 40.0 + np.arange(16); want[ln.IDX["STATUS"]] = 1.0
    assert np.array_equal(recs[0, 1], want) and not seen[4]["metrics"][0].any()
    assert not recs[0, 2].any() and np.array_equal(seen[6]["metrics"][0], 60.0 + np.arange(16))
    # car 1: one driving period, then lost: nothing moves any more
    assert np.array_equal(st[1], [0, 1, 50.0, 0]) and np.isnan(times[1]).all() and not recs[1].any()
    assert all(np.array_equal(d["metrics"][1], 10.0 * c + np.arange(16) + 100.0) for c, d in enumerate(seen))
    # car 2: k = 0 with s >= L: a lap of 0 s, wrapped, and driving from there
    assert times[2, 0] == 0.0 and np.isnan(times[2, 1:]).all() and seen[0]["x0"][2, 0] == 0.5 and seen[0]["fin"][2] == 0
    assert np.array_equal(st[2], [1, 7, 6.0, 0.0]) and recs[2, 0, ln.IDX["STATUS"]] == 1.0 and recs[2, 0, 0] == 200.0
    # car 3: k = 3, s == S_PREV = 99 (not s > S_PREV): f = 1, t = 3 dt; the wrap makes s negative, as the rule says
    assert abs(times[3, 0] - 3 * DT) < 1e-15 and seen[3]["x0"][3, 0] == -1.0 and seen[3]["fin"][3] == 0 and st[3, lp.DONE] == 1
    assert st[3, lp.STEPS] == 7 and st[3, lp.S_PREV] == 99.0
    # the clamp: a previous s beyond the line gives f = 0
    s1, t1_, _ = lp.fresh(1, 2)
    s1[0] = [0, 4, 100.5, 0.0]
    x0 = np.array([[101.0, 0, 0, 0, 0]]); xr = np.zeros((1, N, nx)); xk = np.zeros((1, N, nx)); f1 = np.array([1])
    lp.gate(DT, L, 2, x0, xr, xk, f1, s1, t1_)
    assert abs(t1_[0, 0] - 3 * DT) < 1e-15 and x0[0, 0] == 1.0 and xr[0, 0, 0] == -100.0
    # laps = 1: the first crossing is final, nothing but the time and the state moves
    s1, t1_, _ = lp.fresh(1, 1)
    s1[0] = [0, 2, 98.0, 0.0]
    x0 = np.array([[101.0, 0, 0, 0, 0]]); f1 = np.array([1])
    lp.gate(DT, L, 1, x0, xr, xk, f1, s1, t1_)
    assert x0[0, 0] == 101.0 and f1[0] == 1 and s1[0, lp.DONE] == 1 and s1[0, lp.STEPS] == 2 and abs(t1_[0, 0] - (1 + 2.0 / 3.0) * DT) < 1e-15


def _summary(fm, t, laps):
    t = np.ascontiguousarray(t, dtype=np.float64)
    out = np.full((laps, 4), -777.0)
    rc = fm.lib().fsaempc_cl_lap_summary(C.c_void_p(t.ctypes.data) if t.size else None, t.shape[0], laps, C.c_void_p(out.ctypes.data))
    return rc, out


@pytest.mark.parametrize("case", ["batch 1", "nobody finished", "all finished", "mixed NaN", "empty"])
def test_host_lap_summary_is_numpys(case):
    import fsae_mpc_amd as fm
    rng = np.random.default_rng(17)
    laps = 3
    if case == "batch 1":
        t = np.array([[21.5, 19.25, np.nan]])
    elif case == "nobody finished":
        t = np.full((7, laps), np.nan)
    elif case == "all finished":
        t = rng.uniform(15, 30, (9, laps))
    elif case == "mixed NaN":
        t = rng.uniform(15, 30, (37, laps)); t[rng.uniform(0, 1, 37) > 0.5, 2] = np.nan; t[rng.uniform(0, 1, 37) > 0.8, 1:] = np.nan
    else:
        t = np.zeros((0, laps))
    rc, out = _summary(fm, t, laps)
    assert rc == 0
    want = lp.summary(t)
    assert np.array_equal(np.isnan(out), np.isnan(want)) and np.array_equal(out[:, 0], want[:, 0])
    assert np.allclose(out[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-13, atol=0)
    if case == "batch 1":
        assert np.array_equal(out[0], [1, 21.5, 21.5, 21.5]) and out[2, 0] == 0 and np.isnan(out[2, 1:]).all()
    if case in ("nobody finished", "empty"):
        assert (out[:, 0] == 0).all() and np.isnan(out[:, 1:]).all()
    if case == "mixed NaN":
        assert 0 < out[2, 0] < out[1, 0] < out[0, 0] == 37
    assert np.array_equal(_summary(fm, t, laps)[1], out, equal_nan=True)      # fixed order: the same bits
    # the entry's own refusals
    L = fm.lib()
    o = C.c_void_p(out.ctypes.data)
    assert _summary(fm, t, 0)[0] == -1 and b"laps" in L.fsaempc_last_error()
    assert L.fsaempc_cl_lap_summary(C.c_void_p(out.ctypes.data), 1, 65, o) == -1
    assert L.fsaempc_cl_lap_summary(C.c_void_p(out.ctypes.data), -1, laps, o) == -1
    assert L.fsaempc_cl_lap_summary(None, 2, laps, o) == -1 and L.fsaempc_cl_lap_summary(C.c_void_p(out.ctypes.data), 1, laps, None) == -1
    # LapReport.lap_summary() is the same table
    if t.shape[0]:
        done = (~np.isnan(t)).sum(axis=1)
        st = np.zeros((t.shape[0], 4)); st[:, 0] = done
        rep = fm.LapReport(np.zeros((t.shape[0], 16)), DT, t, st, np.zeros((t.shape[0], laps, 16)))
        assert np.array_equal(rep.lap_summary(), out, equal_nan=True) and np.array_equal(rep.laps_done, done)
        assert np.allclose(rep.lap_time, np.nansum(t, axis=1), rtol=1e-15) and rep.lap_records.shape == (t.shape[0], laps, 16)


def test_lap_report_places_the_live_record():
    import fsae_mpc_amd as fm
    rng = np.random.default_rng(4)
    laps, B = 3, 4
    m = rng.uniform(1, 2, (B, 16)); m[:, 1] = [0, 0, 1, 2]
    recs = np.zeros((B, laps, 16)); recs[1, 0] = 5.0; recs[2, :2] = 6.0
    st = np.zeros((B, 4)); st[:, 0] = [0, 1, 3, 0]
    t = np.full((B, laps), np.nan); t[1, 0] = 20.0; t[2] = [21.0, 19.0, 19.5]
    rep = fm.LapReport(m, DT, t, st, recs)
    assert np.array_equal(rep.lap_records[0, 0], m[0]) and not rep.lap_records[0, 1:].any()
    assert (rep.lap_records[1, 0] == 5.0).all() and np.array_equal(rep.lap_records[1, 1], m[1]) and not rep.lap_records[1, 2].any()
    assert (rep.lap_records[2, :2] == 6.0).all() and np.array_equal(rep.lap_records[2, 2], m[2])      # finished: row laps - 1
    assert np.array_equal(rep.lap_time, [0.0, 20.0, 59.5, 0.0]) and np.array_equal(rep.status, m[:, 1]) and rep.laps == 3
    assert not recs[0, 0].any()                                                                        # the caller's array is not written
    # without the gate's arrays: the single lap under the same names
    one = fm.LapReport(m, DT)
    assert np.array_equal(one.laps_done, [0, 0, 1, 0]) and one.lap_times.shape == (B, 1) and one.lap_times[2, 0] == m[2, 0] * DT
    assert np.isnan(one.lap_times[[0, 1, 3], 0]).all() and np.array_equal(one.lap_records[:, 0], m) and np.array_equal(one.lap_time, m[:, 0] * DT)
    assert np.array_equal(one.lap_summary()[0], [1, m[2, 0] * DT, m[2, 0] * DT, m[2, 0] * DT])


def test_header_macros_match_the_python_tables():
    import fsae_mpc_amd as fm
    hdr = open(os.path.join(ROOT, "include", "fsaempc.h")).read()
    slots = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+FSAEMPC_LS_([A-Z_0-9]+)\s+(\d+)", hdr)}
    assert slots == fm.LAP_STATE_INDEX and list(fm.LAP_STATE_INDEX) == lp.STATE
    assert [fm.LAP_STATE_INDEX[n] for n in lp.STATE] == [lp.DONE, lp.STEPS, lp.S_PREV, lp.T_CROSS]
    assert int(re.search(r"#define\s+FSAEMPC_NLAPSTATE\s+(\d+)", hdr).group(1)) == fm.NLAPSTATE == len(slots) == 4
    assert int(re.search(r"#define\s+FSAEMPC_MAX_LAPS\s+(\d+)", hdr).group(1)) == fm.MAX_LAPS == 64
    for s in ("fsaempc_cl_lap_gate_batch_device", "fsaempc_cl_lap_summary"):
        assert s in fm._lib.EXPORTS and hasattr(fm.lib(), s) and ("int %s(" % s) in hdr, s
    for name in ("LAP_STATE_INDEX", "NLAPSTATE", "MAX_LAPS"):
        assert name in fm.__all__ and hasattr(fm, name)


def test_gate_entry_refuses_bad_arguments_before_any_launch():
    import torch
    import fsae_mpc_amd as fm
    L = fm.lib()
    B, N, laps = 3, 4, 3
    p = lambda a: C.c_void_p(a.data_ptr())
    nan, inf = float("nan"), float("inf")
    for nx in (5, 7):
        f64 = lambda *s: torch.full(s, 7.0, dtype=torch.float64)
        bufs = dict(x0=f64(B, nx), x_ref=f64(B, N, nx), x_keep=f64(B, N, nx), finished=torch.full((B,), 7, dtype=torch.int32), lap_state=f64(B, 4),
                    lap_times=f64(B, laps), metrics=f64(B, 16), lap_records=f64(B, laps, 16))
        order = ["x0", "x_ref", "x_keep", "finished", "lap_state", "lap_times", "metrics", "lap_records"]

        def call(nx_=nx, N_=N, dt=DT, L_=100.0, laps_=laps, batch=B, null=()):
            return L.fsaempc_cl_lap_gate_batch_device(nx_, N_, C.c_double(dt), C.c_double(L_), laps_, batch,
                                                      *[None if k in null else p(bufs[k]) for k in order], None)
        for k in order[:6]:
            assert call(null=(k,)) == -1 and b"null" in L.fsaempc_last_error(), k
        assert call(null=("metrics",)) == -1 and b"together" in L.fsaempc_last_error()
        assert call(null=("lap_records",)) == -1 and b"together" in L.fsaempc_last_error()
        for kw in (dict(laps_=0), dict(laps_=-1), dict(laps_=65)):
            assert call(**kw) == -1 and b"laps" in L.fsaempc_last_error(), kw
        for kw in (dict(nx_=6), dict(nx_=0), dict(nx_=4)):
            assert call(**kw) == -1 and b"nx" in L.fsaempc_last_error(), kw
        for kw in (dict(N_=0), dict(N_=-3), dict(batch=-1), dict(dt=0.0), dict(dt=-DT), dict(dt=nan), dict(dt=inf), dict(L_=0.0), dict(L_=-1.0),
                   dict(L_=nan), dict(L_=inf)):
            assert call(**kw) == -1 and len(L.fsaempc_last_error()) > 0, kw
        assert call(batch=0) == 0 and call(batch=0, null=("metrics", "lap_records")) == 0 and call(batch=0, laps_=64) == 0   # nothing to launch
        assert all(bool((bufs[k] == 7).all()) for k in order)
        if torch.cuda.is_available():
            continue     # the rest states what happens without a device
        assert call() == -4 and call(null=("metrics", "lap_records")) == -4                                # FSAEMPC_ERR_NODEVICE: no CPU path
        assert all(bool((bufs[k] == 7).all()) for k in order)


def test_python_options_are_checked_before_the_library_is_touched():
    import subprocess, sys
    code = """
import sys
sys.path.insert(0, %r)
import fsae_mpc_amd as fm
for laps in (0, 65, -1, 1.5, "two"):
    try:
        fm.ClosedLoop(fm.KINEMATIC, 10, 0.05, None, [[0.0] * 7], laps=laps)
    except ValueError:
        pass
    else:
        raise SystemExit("no ValueError for ClosedLoop(laps = %%r)" %% (laps,))
    try:
        fm.monte_carlo(fm.KINEMATIC, 10, fm.Track.load("fsg2019"), 2, 1, laps=laps)
    except ValueError:
        continue
    raise SystemExit("no ValueError for monte_carlo(laps = %%r)" %% (laps,))
assert fm._lib._LIB is None, "the library was loaded"
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout, out.stderr)


def test_gate_script_of_the_gpu_test_does_what_it_says():
    """GPU test A's five kinds on the restatement: the crossings happen on the calls the kinds name."""
    B = 10
    kind, s, raise_, lost = lp.gate_script(B)
    st, times, _ = lp.fresh(B, lp.GATE_LAPS)
    fin = np.zeros(B, dtype=int)
    done = []
    for call in range(lp.GATE_CALLS):
        x0, x_ref, x_keep, fin = lp.gate_inputs(B, call, s, raise_, lost, fin)
        lp.gate(lp.GATE_DT, lp.GATE_L, lp.GATE_LAPS, x0, x_ref, x_keep, fin, st, times)
        done.append(st[:, lp.DONE].copy())
    done = np.array(done)
    for b in range(B):
        want = {0: [0, 0, 1, 1, 2, 2], 1: [0, 1, 2, 3, 3, 3], 2: [0] * 6, 3: [0] * 6, 4: [1] * 6}[kind[b]]
        assert np.array_equal(done[:, b], want), (b, done[:, b])
    assert (fin[kind == 1] == 1).all() and (fin[kind == 3] == 2).all() and (fin[(kind != 1) & (kind != 3)] == 0).all()
    assert (st[kind == 3] == 0).all() and np.isnan(times[kind == 3]).all() and np.isnan(times[kind == 2]).all()
    assert (times[kind == 4, 0] == 0.0).all() and (~np.isnan(times[kind == 1])).all() and (st[kind == 1, lp.STEPS] == 3).all()
    assert not np.array_equal(times[0], times[5])                      # the per-car offset: no two lanes hold the same numbers


def _no_trouble_around(h, b, flag_ok=(0,)):
    """exit flag 0 on the three steps around every wrap of car b; returns the steps on which the gate wrapped it"""
    ts = np.nonzero(h["crossed"][:, b])[0]
    T = h["flag"].shape[0]
    for t in ts:
        for u in (t - 1, t, t + 1):
            if 0 <= u < T and h["finished"][u, b] == 0:
                assert h["flag"][u, b] in flag_ok, (b, t, u, h["flag"][u, b])
    return ts


def test_inputs_vetted_on_the_oracle_one_crossing(orc, otrack):
    """The cars of GPU test C (lap_numpy.cars on fsg2019, kinematic N = 10, laps = 2, 30 steps) on the oracle's closed loop with the
    restated gate: the near-end car crosses once, within 4 .. 6 steps, drives on to step 30 with |n| continuous across the wrap; no other car
    crosses; nobody is lost after a wrap."""
    cart, s0, v0, kind = ln.cars(otrack, 5)
    h, st, times = lp.drive_oracle_laps(orc, otrack, 0, 10, DT, cart, s0, v0, 30, 2)
    assert np.array_equal(st[:, lp.DONE], [0, 0, 1, 0, 0]) and np.array_equal(h["finished"][-1], [0, 0, 0, 2, 0])
    ts = _no_trouble_around(h, 2)
    assert len(ts) == 1 and 4 <= ts[0] <= 6 and h["crossed"].sum() == 1
    t = ts[0]
    assert abs(abs(h["x0"][t, 2, 1]) - abs(h["x0"][t - 1, 2, 1])) < 0.05 and abs(abs(h["x0"][t + 1, 2, 1]) - abs(h["x0"][t, 2, 1])) < 0.05
    assert 0 < h["x0"][t, 2, 0] < 2 and 0 < h["x0"][t + 1, 2, 0] < 2 and st[2, lp.STEPS] == 30
    assert (t - 1) * DT < times[2, 0] <= t * DT and np.isnan(times[2, 1])
    assert (h["flag"][:, 2] == 0).all()


def test_inputs_vetted_on_the_oracle_short_track(orc):
    """The cars of GPU test E (laps_numpy.circle_starts on the circle of laps_numpy.CIRCLE, kinematic N = 10, laps = 3, 300 steps) on the
    oracle's closed loop with the restated gate: two crossings per car within the cap, nobody lost, exit flag 0 around every crossing, and
    the flying lap within 2 % of L / mean speed."""
    import fsae_mpc_amd as fm
    c = lp.CIRCLE
    tr = fm.Track.from_points(*lp.circle_points(), M=c["M"])
    otr = orc.Track(tr.xP, tr.yP, tr.dl, tr.L)
    assert abs(tr.L - 2 * np.pi * c["radius"]) < 0.05
    cart, s0, v0, kind = ln.cars(otr, c["B"], lp.circle_starts(tr.L))
    h, st, times = lp.drive_oracle_laps(orc, otr, 0, c["N"], DT, cart, s0, v0, c["cap"], c["laps"], target_vel=c["target_vel"])
    print("short track: L", tr.L, "laps done", st[:, lp.DONE], "lap times", times)
    assert (st[:, lp.DONE] == 2).all() and (h["finished"] == 0).all()
    for b in range(c["B"]):
        ts = _no_trouble_around(h, b)
        assert len(ts) == 2 and ts[0] < 30, (b, ts)
        v = h["x0"][ts[0]:ts[1], b, 3]
        assert abs(times[b, 1] - tr.L / v.mean()) <= 0.02 * times[b, 1], (b, times[b, 1], tr.L / v.mean())
    assert (st[:, lp.STEPS] == c["cap"]).all()
