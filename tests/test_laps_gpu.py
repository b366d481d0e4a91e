"""GPU tests of the multi-lap closed loop.  The lap gate is compared, call by call, with its numpy restatement
(tests/laps_numpy.py): x0, x_ref, the kept plan, `finished`, the live record and the handed-over records bit for bit (subtracting L is one
IEEE operation on both sides, the rest are copies), lap_state and lap_times to 1e-12 absolute -- the values are O(100 s) at most and the chain
is a few operations in which the compiler may contract (k - 1 + f) dt - T into a fused multiply-add; a wrong or missing term is at least
1e-3 dt = 5e-5.  The records are compared with tests/lap_numpy.py's restatement of the lap report, with the tolerances of
tests/test_lap_report_gpu.py.  The cars and the short track are vetted on the oracle in tests/test_laps_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import lap_numpy as ln
import laps_numpy as lp

pytestmark = pytest.mark.gpu

DT = 0.05
TOL_T = 1e-12
TOL = 1e-10
I = ln.IDX


@pytest.fixture(scope="module")
def fm():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd
    return fsae_mpc_amd


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def tr(fm):
    return fm.Track.load("fsg2019")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _close(a, b, tol):
    """NaN in the same places, the rest within tol absolute; returns the worst deviation"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    d = np.abs(a - b)[~np.isnan(b)]
    worst = float(d.max()) if d.size else 0.0
    assert worst <= tol, worst
    return worst


# ---- A, B. the gate alone ----------------------------------------------------------------------------------------------------------
def _gate_alone(fm, torch, with_records):
    """Six calls of the entry on 65 hand-made cars beside the restatement, which carries its own state from call to call.  Returns per call
    what each side left, and the kinds."""
    B, laps = 65, lp.GATE_LAPS
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    kind, s, raise_, lost = lp.gate_script(B)
    st, times, recs = lp.fresh(B, laps, metrics=with_records)
    d_st, d_times, d_recs = dev(st), dev(times), (dev(recs) if with_records else None)
    fin = np.zeros(B, dtype=np.int32)
    calls = []
    for call in range(lp.GATE_CALLS):
        x0, x_ref, x_keep, fin = lp.gate_inputs(B, call, s, raise_, lost, fin)
        fin = fin.astype(np.int32)
        metrics = (1000.0 * (call + 1) + 16.0 * np.arange(B)[:, None] + np.arange(16)[None, :] + 0.5) if with_records else None
        before = dict(x0=x0.copy(), x_ref=x_ref.copy(), x_keep=x_keep.copy(), fin=fin.copy(), st=d_st.cpu().numpy(), times=d_times.cpu().numpy(),
                      metrics=None if metrics is None else metrics.copy(), recs=d_recs.cpu().numpy() if with_records else None)
        d = dict(x0=dev(x0), x_ref=dev(x_ref), x_keep=dev(x_keep), fin=dev(fin), metrics=dev(metrics) if with_records else None)
        rc = fm.lib().fsaempc_cl_lap_gate_batch_device(lp.GATE_NX, lp.GATE_N, C.c_double(lp.GATE_DT), C.c_double(lp.GATE_L), laps, B, p(d["x0"]),
                                                       p(d["x_ref"]), p(d["x_keep"]), p(d["fin"]), p(d_st), p(d_times), p(d["metrics"]), p(d_recs),
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, fm.lib().fsaempc_last_error()
        torch.cuda.synchronize()
        lp.gate(lp.GATE_DT, lp.GATE_L, laps, x0, x_ref, x_keep, fin, st, times, metrics, recs)
        got = dict(x0=d["x0"].cpu().numpy(), x_ref=d["x_ref"].cpu().numpy(), x_keep=d["x_keep"].cpu().numpy(), fin=d["fin"].cpu().numpy(),
                   st=d_st.cpu().numpy(), times=d_times.cpu().numpy(), metrics=d["metrics"].cpu().numpy() if with_records else None,
                   recs=d_recs.cpu().numpy() if with_records else None)
        want = dict(x0=x0.copy(), x_ref=x_ref.copy(), x_keep=x_keep.copy(), fin=fin.copy(), st=st.copy(), times=times.copy(),
                    metrics=None if metrics is None else metrics.copy(), recs=None if recs is None else recs.copy())
        calls.append((before, got, want))
    return kind, calls


def test_a_gate_alone_full_wavefront_plus_one(fm, torch_):
    kind, calls = _gate_alone(fm, torch_, False)
    worst = 0.0
    for call, (before, got, want) in enumerate(calls):
        for k in ("x0", "x_ref", "x_keep", "fin"):
            assert _bits(got[k], want[k]), (call, k, np.nonzero((got[k] != want[k]).reshape(65, -1).any(axis=1))[0])
        worst = max(worst, _close(got["st"], want["st"], TOL_T), _close(got["times"], want["times"], TOL_T))
        # cars the rules say to leave alone keep every bit: the lost ones always, the car past its final crossing on calls 4 and 5
        alone = (kind == 3) | ((kind == 1) & (call >= 4))
        for k in ("x0", "x_ref", "x_keep", "fin", "st", "times"):
            assert _bits(got[k][alone], before[k][alone]), (call, k)
        assert (got["fin"][kind == 3] == 2).all()
    print("A: worst deviation of a time or a state slot", worst)
    before, got, want = calls[-1]
    assert np.array_equal(got["st"][:, lp.DONE], np.array([2, 3, 0, 0, 1])[kind])
    assert np.array_equal(got["fin"], np.array([0, 1, 0, 2, 0])[kind])
    done = ~np.isnan(got["times"])
    assert np.array_equal(done.sum(axis=1), got["st"][:, lp.DONE]) and (got["times"][kind == 4, 0] == 0.0).all()
    # the lane past the wave boundary is its mirror in the first wave again (the script's offsets repeat after twelve groups of five)
    for call, (before, got, want) in enumerate(calls):
        assert kind[64] == kind[4] and got["fin"][64] == got["fin"][4] and _bits(got["st"][64], got["st"][4]) and _bits(got["times"][64], got["times"][4])
        assert got["x0"][64, 0] == got["x0"][4, 0] and _bits(got["x_ref"][64, :, 0], got["x_ref"][4, :, 0]), call
        assert _bits(got["x_keep"][64, :, 0], got["x_keep"][4, :, 0]), call
    assert not _bits(calls[-1][1]["times"][0], calls[-1][1]["times"][5])      # ... and differ between neighbouring groups


def test_b_records_handed_over(fm, torch_):
    kind, calls = _gate_alone(fm, torch_, True)
    crossings = 0
    for call, (before, got, want) in enumerate(calls):
        for k in ("x0", "x_ref", "x_keep", "fin", "metrics", "recs"):
            assert _bits(got[k], want[k]), (call, k)
        _close(got["st"], want["st"], TOL_T); _close(got["times"], want["times"], TOL_T)
        d0, d1 = before["st"][:, lp.DONE].astype(int), got["st"][:, lp.DONE].astype(int)
        for b in range(65):
            if d1[b] == d0[b] or d1[b] == lp.GATE_LAPS:      # no crossing, or the final one: both untouched
                assert _bits(got["metrics"][b], before["metrics"][b]) and _bits(got["recs"][b], before["recs"][b]), (call, b)
                continue
            crossings += 1
            r = before["metrics"][b].copy(); r[I["STATUS"]] = 1.0
            assert _bits(got["recs"][b, d0[b]], r) and not got["metrics"][b].any(), (call, b)
            others = [l for l in range(lp.GATE_LAPS) if l != d0[b]]
            assert _bits(got["recs"][b, others], before["recs"][b, others]), (call, b)
    assert crossings == 13 * (2 + 2 + 1)
    final = [(c, b) for c, (bf, g, w) in enumerate(calls) for b in range(65) if g["st"][b, lp.DONE] == lp.GATE_LAPS > bf["st"][b, lp.DONE]]
    assert len(final) == 13 and all(c == 3 and kind[b] == 1 for c, b in final)
    assert not calls[-1][1]["recs"][:, lp.GATE_LAPS - 1].any()            # the last lap's record is never the gate's to write


# ---- C. in the loop, one crossing --------------------------------------------------------------------------------------------------
GATE_KEYS = ("x0", "x_ref", "x_opt", "finished", "lap_state", "lap_times", "metrics", "lap_records")


def _run(fm, torch, tr, model, N, cart, s0, v0, steps, **kw):
    """The loop of fm.monte_carlo on given cars with cl.lap_gate wrapped: the gate's tensors before and after every call, and the inputs
    of the metrics kernel of every step, kept on the device and read back at the end."""
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    snaps = []
    inner = cl.lap_gate

    def wrapped(stream=None):
        grab = lambda: {k: (getattr(cl, k).clone() if getattr(cl, k) is not None else None) for k in GATE_KEYS}
        before = grab()
        inner(stream)
        snaps.append((before, grab()))
    cl.lap_gate = wrapped
    keep = dict(x0=[], finished=[], flag=[], iter=[], fval=[], slack=[], a=[], cart=[])
    for t in range(steps):
        out = cl.step()
        for k, v in (("x0", cl.x0), ("finished", cl.finished), ("flag", out["exitflag"]), ("iter", out["iter"]), ("fval", out["fval"]),
                     ("slack", out["slack"]), ("a", cl.u_opt[:, 0, 0]), ("cart", cl.cart)):
            keep[k].append(v.clone())
    torch.cuda.synchronize(cl.device)
    h = {k: torch.stack(v).cpu().numpy() for k, v in keep.items()}
    h["slack"] = h["slack"].reshape(steps, cl.B, -1)
    host = lambda d: {k: (v.cpu().numpy() if v is not None else None) for k, v in d.items()}
    return cl, h, [(host(b), host(a)) for b, a in snaps]


def _restate_calls(snaps, L, laps):
    """every call of the gate in the loop against the restatement started from what the device held before it; returns (T, B) wrapped"""
    worst, wrapped = 0.0, []
    for call, (before, after) in enumerate(snaps):
        w = {k: (None if v is None else v.copy()) for k, v in before.items()}
        lp.gate(DT, L, laps, w["x0"], w["x_ref"], w["x_opt"], w["finished"], w["lap_state"], w["lap_times"], w["metrics"], w["lap_records"])
        for k in ("x0", "x_ref", "x_opt", "finished", "metrics", "lap_records"):
            assert (w[k] is None and after[k] is None) or _bits(after[k], w[k]), (call, k)
        worst = max(worst, _close(after["lap_state"], w["lap_state"], TOL_T), _close(after["lap_times"], w["lap_times"], TOL_T))
        wrapped.append((after["lap_state"][:, lp.DONE] > before["lap_state"][:, lp.DONE]) & (after["finished"] == 0))
    return worst, np.array(wrapped)


def _one_crossing(fm, torch, tr, otrack, B, **kw):
    steps, laps = 30, 2
    cart, s0, v0, kind = ln.cars(otrack, B)
    cl, h, snaps = _run(fm, torch, tr, fm.KINEMATIC, 10, cart, s0, v0, steps, metrics=True, laps=laps, **kw)
    assert len(snaps) == steps and tuple(cl.lap_state.shape) == (B, 4) and tuple(cl.lap_times.shape) == (B, laps)
    assert tuple(cl.lap_records.shape) == (B, laps, 16)
    worst, wrapped = _restate_calls(snaps, tr.L, laps)
    rep = cl.report()
    m, recs, st, times = cl.metrics.cpu().numpy(), cl.lap_records.cpu().numpy(), cl.lap_state.cpu().numpy(), cl.lap_times.cpu().numpy()
    fin = cl.finished.cpu().numpy()
    worst_sum = 0.0
    for b in range(B):
        name = ln.CAR_NAMES[kind[b]]
        ts = np.nonzero(wrapped[:, b])[0]
        if name != "near end":
            assert len(ts) == 0 and st[b, lp.DONE] == 0 and np.isnan(times[b]).all() and not recs[b].any(), (b, name)
            worst_sum = max(worst_sum, ln.compare(m[b], ln.car_record(h, b, DT, 1e-6), TOL))
            assert rep.laps_done[b] == 0 and _bits(rep.lap_records[b, 0], m[b]) and not rep.lap_records[b, 1].any() and rep.lap_time[b] == 0.0
            continue
        assert len(ts) == 1 and 4 <= ts[0] <= 6, (b, ts)
        t = int(ts[0])
        assert fin[b] == 0 and st[b, lp.DONE] == 1 and rep.laps_done[b] == 1 and st[b, lp.STEPS] == steps
        assert abs(abs(h["x0"][t, b, 1]) - abs(h["x0"][t - 1, b, 1])) < 0.05, (b, h["x0"][t - 1:t + 2, b, 1])
        assert 0.0 < h["x0"][t + 1, b, 0] < 2.0 and h["x0"][t - 1, b, 0] < tr.L, (b, h["x0"][t - 1:t + 2, b, 0])
        assert (t - 1) * DT < times[b, 0] <= t * DT and np.isnan(times[b, 1]) and rep.lap_time[b] == times[b, 0]
        first = {k: v[:t] for k, v in h.items()}
        want0 = ln.car_record(first, b, DT, 1e-6); want0[I["STATUS"]] = 1.0
        worst_sum = max(worst_sum, ln.compare(recs[b, 0], want0, TOL))
        worst_sum = max(worst_sum, ln.compare(m[b], ln.car_record({k: v[t:] for k, v in h.items()}, b, DT, 1e-6), TOL))
        assert recs[b, 0, I["STEPS"]] + m[b, I["STEPS"]] == steps and not recs[b, 1].any()
        assert _bits(rep.lap_records[b, 0], recs[b, 0]) and _bits(rep.lap_records[b, 1], m[b])
    s = rep.lap_summary()
    near = kind == 2
    assert s.shape == (laps, 4) and s[0, 0] == near.sum() and s[1, 0] == 0 and np.isnan(s[1, 1:]).all()
    assert abs(s[0, 1] - times[near, 0].mean()) < 1e-12 and s[0, 2] == times[near, 0].min() and s[0, 3] == times[near, 0].max()
    return worst, worst_sum, m, recs, times


def test_c_one_crossing_in_the_loop(fm, torch_, tr, otrack):
    worst, worst_sum, m, recs, times = _one_crossing(fm, torch_, tr, otrack, 65)
    print("C: worst deviation of a time or a state slot", worst, "of a sum of a record", worst_sum)
    assert _bits(m[64], m[4]) and _bits(recs[62], recs[2]) and _bits(times[62], times[2])     # past the wave boundary: the same cars again


def test_c_one_crossing_in_a_corridor(fm, torch_, tr, otrack):
    worst, worst_sum, *_ = _one_crossing(fm, torch_, tr, otrack, 8, corridor=fm.Corridor.constant(tr.L, 0.75))
    print("C (corridor): worst deviation of a time or a state slot", worst, "of a sum of a record", worst_sum)


def test_c_one_crossing_on_a_plan(fm, torch_, tr, otrack):
    worst, worst_sum, *_ = _one_crossing(fm, torch_, tr, otrack, 8, reference=fm.Plan.profile(fm.KINEMATIC, tr, N_s=200))
    print("C (plan): worst deviation of a time or a state slot", worst, "of a sum of a record", worst_sum)


# ---- D. laps = 1 is the loop as it was ---------------------------------------------------------------------------------------------
def test_d_one_lap_is_the_loop_as_it_was(fm, torch_, tr, otrack):
    """8 cars, 12 steps (the near-end cars finish within them).  Without laps, with laps=1, and with laps=1 and the gate called all the
    same after every pre-step: the same bits, and nothing allocated unless the gate ran.  laps=2 on the cars that never cross (the near-end
    cars moved to s0 = 20): the same bits as their single-lap run."""
    torch = torch_
    cart, s0, v0, kind = ln.cars(otrack, 8)
    st = ln.starts(otrack); st[2] = (20.0, 0.3, 9.0)
    cart_n, s0_n, v0_n, _ = ln.cars(otrack, 8, st)

    def run(cart, s0, v0, gate_too=False, **kw):
        cl = fm.ClosedLoop(fm.KINEMATIC, 10, DT, tr, cart, metrics=True, **kw)
        cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
        cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
        if gate_too:
            pre = cl.pre
            cl.pre = lambda stream=None: (pre(stream), cl.lap_gate(stream))
        for _ in range(12):
            cl.step()
        torch.cuda.synchronize(cl.device)
        return cl, [getattr(cl, k).cpu().numpy() for k in ("cart", "x_opt", "u_opt", "metrics", "finished")]

    plain, a = run(cart, s0, v0)
    one, b = run(cart, s0, v0, laps=1)
    gated, c = run(cart, s0, v0, gate_too=True, laps=1)
    for x, y, z in zip(a, b, c):
        assert _bits(x, y) and _bits(x, z)
    assert a[4][2] == 1 and a[4][3] == 2
    for cl in (plain, one):
        assert cl.laps == 1 and cl.lap_state is None and cl.lap_times is None and cl.lap_records is None
    # with the gate run at laps = 1: the lap time to a fraction of dt beside STEPS dt, the record latched by the metrics kernel as ever
    t, m = gated.lap_times.cpu().numpy(), c[3]
    assert tuple(t.shape) == (8, 1) and np.array_equal(~np.isnan(t[:, 0]), a[4] == 1) and not gated.lap_records.cpu().numpy().any()
    near = np.nonzero(a[4] == 1)[0]
    assert ((m[near, I["STEPS"]] - 1) * DT < t[near, 0]).all() and (t[near, 0] <= m[near, I["STEPS"]] * DT).all() and (m[near, I["STATUS"]] == 1).all()
    rep = gated.report()
    assert np.array_equal(rep.laps_done, (a[4] == 1).astype(int)) and _bits(rep.lap_records[:, 0], m)
    never1, d = run(cart_n, s0_n, v0_n)
    never2, e = run(cart_n, s0_n, v0_n, laps=2)
    for x, y in zip(d, e):
        assert _bits(x, y)
    assert (e[4][[0, 1, 2, 4, 5, 6, 7]] == 0).all() and never2.lap_state.cpu().numpy()[:, lp.DONE].max() == 0
    assert np.array_equal(never2.lap_state.cpu().numpy()[:, lp.STEPS], np.where(e[4] == 0, 12.0, 0.0))
    # monte_carlo passes the option through
    out = fm.monte_carlo(fm.KINEMATIC, 10, tr, 8, 2, laps=3)
    assert out[0].laps == 3 and tuple(out[0].lap_times.shape) == (8, 3) and out[0].lap_records is None


# ---- E. two crossings on a short closed track --------------------------------------------------------------------------------------
_SHORT = {}


def _short_track_run(fm, torch):
    c = lp.CIRCLE
    trk = fm.Track.from_points(*lp.circle_points(), M=c["M"])
    import oracle
    otr = oracle.Track(trk.xP, trk.yP, trk.dl, trk.L)           # (the table holder alone: lap_numpy.cart_on_track reads it)
    cart, s0, v0, kind = ln.cars(otr, c["B"], lp.circle_starts(trk.L))
    cl = fm.ClosedLoop(fm.KINEMATIC, c["N"], DT, trk, cart, target_vel=c["target_vel"], metrics=True, laps=c["laps"])
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    x0s, dones = [], []
    for t in range(c["cap"]):
        cl.step()
        x0s.append(cl.x0.clone()); dones.append(cl.lap_state[:, lp.DONE].clone())
    torch.cuda.synchronize(cl.device)
    return trk, cl, torch.stack(x0s).cpu().numpy(), torch.stack(dones).cpu().numpy()


def test_e_two_crossings_on_a_short_track(fm, torch_):
    c = lp.CIRCLE
    trk, cl, x0, done = _short_track_run(fm, torch_)
    rep = cl.report()
    times, fin = cl.lap_times.cpu().numpy(), cl.finished.cpu().numpy()
    print("E: L", trk.L, "laps done", rep.laps_done, "lap times", times)
    assert (fin != 2).all() and (rep.laps_done >= 2).all()
    for b in range(c["B"]):
        t1, t2 = int(np.argmax(done[:, b] >= 1)), int(np.argmax(done[:, b] >= 2))
        v = x0[t1:t2, b, 3]                                     # the speeds recorded over the flying lap
        want = trk.L / v.mean()
        print("E: car", b, "flying lap", times[b, 1], "L / mean speed", want, "steps", t2 - t1)
        assert abs(times[b, 1] - want) <= 0.02 * want, (b, times[b, 1], want)
        assert abs(times[b, 1] - (t2 - t1) * DT) <= DT                # and the two crossing steps bracket it
    steps = rep.lap_records[:, :, I["STEPS"]].sum(axis=1)
    driven = cl.lap_state.cpu().numpy()[:, lp.STEPS]
    assert np.array_equal(steps, driven) and (driven[fin == 0] == c["cap"]).all()
    assert (rep.lap_records[:, :2, I["STATUS"]] == 1).all()
    # two runs give the same bits
    _, cl2, x0_2, _ = _short_track_run(fm, torch_)
    for k in ("cart", "x_opt", "u_opt", "metrics", "lap_state", "lap_times", "lap_records", "finished"):
        assert _bits(getattr(cl, k).cpu().numpy(), getattr(cl2, k).cpu().numpy()), k
    assert _bits(x0, x0_2)
