"""GPU tests of the lap report.  Every test reads back, step by step, the data that fed the accumulation kernel (x0,
finished, exit flags, iterations, fval, slack, the first acceleration of the driven plan, the post-plant state), accumulates it with the
numpy restatement (tests/lap_numpy.py) and compares with cl.metrics: count slots and STATUS exactly, the sums to 1e-10 absolute plus
relative -- each sum has at most 30 terms of size O(1 .. 100), each correct to a few ulp; the only arithmetic that differs between the
two sides is exp / atan / sin in Fcr; a missing or misplaced term is at least 1e-4.  The cars are vetted on the oracle in
tests/test_lap_report_cpu.py::test_inputs_vetted_on_the_oracle."""
import numpy as np
import pytest

import lap_numpy as ln

pytestmark = pytest.mark.gpu

DT = 0.05
TOL = 1e-10
I = ln.IDX
_RUNS = {}


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


def _run(fm, torch, tr, model, N, cart, s0, v0, steps, before=None, after=None, **kw):
    """The loop of fm.monte_carlo on given cars, with the kernel's inputs of every step kept on the device and read back at the end.
    before(t, cl) / after(t, cl, out): hooks around step t."""
    cl = fm.ClosedLoop(model, N, DT, tr, cart, **kw)
    cl.x_opt[:, :, 0] += torch.from_numpy(s0).to(cl.device)[:, None]
    cl.x_opt[:, :, 3] += torch.from_numpy(v0).to(cl.device)[:, None]
    keep = dict(x0=[], finished=[], flag=[], iter=[], fval=[], slack=[], a=[], cart=[])
    for t in range(steps):
        if before is not None:
            before(t, cl)
        out = cl.step()
        if after is not None:
            after(t, cl, out)
        for k, v in (("x0", cl.x0), ("finished", cl.finished), ("flag", out["exitflag"]), ("iter", out["iter"]), ("fval", out["fval"]),
                     ("slack", out["slack"]), ("a", cl.u_opt[:, 0, 0]), ("cart", cl.cart)):
            keep[k].append(v.clone())
    torch.cuda.synchronize(cl.device)
    h = {k: torch.stack(v).cpu().numpy() for k, v in keep.items()}
    h["slack"] = h["slack"].reshape(steps, cl.B, -1)
    return cl, h


def _run_a(fm, torch, tr, otrack):
    """test A's run, made once and left unchanged"""
    if "A" not in _RUNS:
        cart, s0, v0, kind = ln.cars(otrack, 65)
        cl, h = _run(fm, torch, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True)
        m = cl.metrics.cpu().numpy(); m.setflags(write=False)
        for v in h.values():
            v.setflags(write=False)
        _RUNS["A"] = (m, h, kind, cl.report())
    return _RUNS["A"]


def test_a_kinematic_full_wavefront_plus_one(fm, torch_, tr, otrack):
    m, h, kind, rep = _run_a(fm, torch_, tr, otrack)
    assert m.shape == (65, 16)
    want = ln.records(h, DT, 1e-6)
    print("A: worst deviation of a sum", ln.compare(m, want, TOL))
    for b in range(65):
        r, name = m[b], ln.CAR_NAMES[kind[b]]
        if name == "off-line":
            assert r[I["N_VIOL_INT"]] > 0 and r[I["SLACK_N_CNT"]] > 0 and r[I["STATUS"]] == 0 and r[I["STEPS"]] == 30, b
        elif name == "near end":
            assert r[I["STATUS"]] == 1 and 4 <= r[I["STEPS"]] <= 6 and r[I["STEPS"]] == want[b, I["STEPS"]], b
        elif name == "lost":
            assert r[I["STATUS"]] == 2 and r[I["STEPS"]] == 0 and np.count_nonzero(r) == 1, b
        elif name == "centre":
            assert r[I["N_VIOL_INT"]] == 0 and r[I["STATUS"]] == 0 and r[I["OBJ_CNT"]] > 0, b
    assert np.array_equal(m[64], m[4])                      # the lane past the wave boundary is the mirror car again
    # report(): the same records by name, and the summary of the host entry
    assert np.array_equal(rep.metrics, m) and np.array_equal(rep.status, m[:, I["STATUS"]]) and np.array_equal(rep.lap_time, m[:, I["STEPS"]] * DT)
    s, ws = rep.summary(), ln.summary(m, DT)
    for k in ln.SUMMARY:
        assert abs(s[k.lower()] - ws[k]) <= 1e-12 * max(1.0, abs(ws[k])), k
    assert s["cars_finished"] == 13 and s["cars_lost"] == 13 and s["cars_driving"] == 39


def test_b_shared_block_with_a_small_ellipse(fm, torch_, tr, otrack):
    cart, s0, v0, kind = ln.cars(otrack, 8)
    P = fm.default_params(fm.KINEMATIC); P[fm.PARAM_INDEX["ELL_LONG"]] = 1.0; P[fm.PARAM_INDEX["ELL_LAT"]] = 2.0
    cl, h = _run(fm, torch_, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True, params=P)
    m = cl.metrics.cpu().numpy()
    print("B: worst deviation of a sum", ln.compare(m, ln.records(h, DT, 1e-6, P), TOL))
    off = m[1]
    assert off[I["ELL_VIOL_INT"]] > 0 and off[I["ELL_VIOL_MAX"]] > 1
    # (the kinematic QP has no ellipse rows: these axes change the report alone)
    assert np.array_equal(m[:, I["STATUS"]], [0, 0, 1, 2, 0, 0, 0, 1])


def test_c_dynamic_per_car_blocks(fm, torch_, tr, otrack):
    st = ln.starts(otrack)
    st = [(20.0, 0.6, 8.0), (20.0, 0.6, 8.0)] + st + [(40.0, -0.3, 6.0)]
    cart, s0, v0, kind = ln.cars(otrack, 8, st)
    P = np.repeat(fm.default_params(fm.DYNAMIC)[None], 8, axis=0)
    P[1, fm.PARAM_INDEX["N_MAX"]] = 0.5
    cl, h = _run(fm, torch_, tr, fm.DYNAMIC, 10, cart, s0, v0, 20, metrics=True, params=P)
    m = cl.metrics.cpu().numpy()
    print("C: worst deviation of a sum", ln.compare(m, ln.records(h, DT, 1e-6, P), TOL))
    assert m[0, I["N_VIOL_INT"]] == 0 and m[0, I["N_VIOL_MAX"]] == 0 and m[0, I["N_ABS_MAX"]] >= 0.59
    assert m[1, I["N_VIOL_INT"]] > 0 and abs(m[1, I["N_VIOL_MAX"]] - 0.1) <= 1e-6 and m[1, I["N_ABS_MAX"]] >= 0.59
    drove = h["finished"] == 0
    assert np.array_equal(m[:, I["SLACK_TYRE_CNT"]], ((h["slack"][:, :, 3] > 1e-6) & drove).sum(axis=0))
    assert np.array_equal(m[:, I["SLACK_N_CNT"]], ((h["slack"][:, :, 0] > 1e-6) & drove).sum(axis=0))


def test_d_the_loop_is_unchanged_with_and_without_metrics(fm, torch_, tr, otrack):
    cart, s0, v0, kind = ln.cars(otrack, 8)
    got = []
    for metrics in (False, True):
        cl = fm.ClosedLoop(fm.KINEMATIC, 10, DT, tr, cart, metrics=metrics)
        cl.x_opt[:, :, 0] += torch_.from_numpy(s0).to(cl.device)[:, None]
        cl.x_opt[:, :, 3] += torch_.from_numpy(v0).to(cl.device)[:, None]
        flags = []
        for _ in range(10):
            out = cl.step()
            flags.append(torch_.stack([out["exitflag"], out["iter"]]).clone())
        torch_.cuda.synchronize(cl.device)
        assert (cl.metrics is None) == (not metrics)
        got.append([cl.cart.cpu().numpy(), cl.x_opt.cpu().numpy(), cl.u_opt.cpu().numpy(), torch_.stack(flags).cpu().numpy(),
                    cl.finished.cpu().numpy()])
        if not metrics:
            with pytest.raises(ValueError):
                cl.report()
        else:
            assert tuple(cl.metrics.shape) == (8, 16) and float(cl.metrics[:, I["STEPS"]].max()) == 10.0
    for x, y in zip(*got):
        assert x.tobytes() == y.tobytes()


def test_e_move_blocking_and_a_plan(fm, torch_, tr, otrack):
    cart, s0, v0, kind = ln.cars(otrack, 8)
    plan = fm.Plan.profile(fm.KINEMATIC, tr, N_s=200)
    cl, h = _run(fm, torch_, tr, fm.KINEMATIC, 10, cart, s0, v0, 15, metrics=True, blocking=[2] * 5, reference=plan)
    m = cl.metrics.cpu().numpy()
    print("E: worst deviation of a sum", ln.compare(m, ln.records(h, DT, 1e-6), TOL))
    assert m[3, I["STATUS"]] == 2 and m[0, I["STEPS"]] == 15 and m[1, I["N_VIOL_INT"]] > 0
    # monte_carlo passes the option through and keeps its return tuple
    out = fm.monte_carlo(fm.KINEMATIC, 10, tr, 8, 3, metrics=True)
    assert len(out) == 4 and tuple(out[0].metrics.shape) == (8, 16) and out[0].report().steps.max() == 3
    assert fm.monte_carlo(fm.KINEMATIC, 10, tr, 8, 1)[0].metrics is None


def test_f_two_runs_give_the_same_bits(fm, torch_, tr, otrack):
    m, h, kind, rep = _run_a(fm, torch_, tr, otrack)
    cart, s0, v0, _ = ln.cars(otrack, 65)
    cl, h2 = _run(fm, torch_, tr, fm.KINEMATIC, 10, cart, s0, v0, 30, metrics=True)
    assert cl.metrics.cpu().numpy().tobytes() == m.tobytes()


def test_g_a_rejected_plan_is_not_what_the_report_reads(fm, torch_, tr, otrack):
    """The acceleration in the ellipse value is that of the plan the car drives on, not of what the solver returned.  No test car ever has
    a plan rejected, so one is made: before step 4 one entry of the off-line car's linearisation point (the n of stage 5, not a set point of
    the plant) is NaN, so that step's QP has non-finite data, the solve returns flag -1 with iter = 0 for it alone, the hand-over keeps
    the plan of step 3 and the car drives on; the entry is put back afterwards.  With ELL_LONG = 1 the kept acceleration gives e > 1
    on that step; what the solver returned does not equal it."""
    cart, s0, v0, kind = ln.cars(otrack, 8)
    P = fm.default_params(fm.KINEMATIC); P[fm.PARAM_INDEX["ELL_LONG"]] = 1.0; P[fm.PARAM_INDEX["ELL_LAT"]] = 2.0
    seen = {}

    def before(t, cl):
        if t == 4:
            seen["saved"] = cl.x_opt[1, 5, 1].clone()
            seen["a_kept"] = cl.u_opt[1, 0, 0].clone()
            cl.x_opt[1, 5, 1] = float("nan")

    def after(t, cl, out):
        if t == 4:
            seen["a_solver"] = out["u_opt"][1, 0].clone()
            seen["flag"] = out["exitflag"][1].clone()
            cl.x_opt[1, 5, 1] = seen["saved"]

    cl, h = _run(fm, torch_, tr, fm.KINEMATIC, 10, cart, s0, v0, 12, before=before, after=after, metrics=True, params=P)
    m = cl.metrics.cpu().numpy()
    a_kept, a_solver, flag = float(seen["a_kept"]), float(seen["a_solver"]), int(seen["flag"])
    print("G: flag", flag, "kept a", a_kept, "solver's a", a_solver)
    assert flag not in (0, 1) and h["flag"][4, 1] == flag and (h["flag"][4, [0, 2, 4, 5, 6, 7]] == 0).all()   # the other cars are unaffected
    assert h["a"][4, 1] == a_kept and not (a_solver == a_kept) and a_kept ** 2 > 1.0 and h["finished"][11, 1] == 0
    want = ln.records(h, DT, 1e-6, P)
    print("G: worst deviation of a sum", ln.compare(m, want, TOL))
    assert m[1, I["ABNORMAL"]] >= 1 and m[1, I["STEPS"]] == 12 and m[1, I["OBJ_CNT"]] <= 11
    # the same history with the solver's acceleration on that step is a different record: the comparison above pins the wiring
    h2 = dict(h); h2["a"] = h["a"].copy(); h2["a"][4, 1] = a_solver if np.isfinite(a_solver) else 0.0
    other = ln.car_record(h2, 1, DT, 1e-6, P)
    assert abs(other[I["ELL_VIOL_INT"]] - m[1, I["ELL_VIOL_INT"]]) > 1e-4
