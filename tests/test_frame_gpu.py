"""The three kernels every closed-loop feature stands on -- cl_pre_kernel, cl_plant_kernel, cl_accept_kernel (csrc/plant.hip,
csrc/cl_frame.h) -- and the frame part of cl_pre_plan_kernel (csrc/planner.hip) against the long-double run of tests/frame_numpy.py, a
restatement written from the reference's files, on the case tables of tests/frame_cases.py: the angdiff wrap, poor and out-of-range
Newton guesses, the lap check at s = L, both sides of every out-of-race threshold, blown-up and non-finite states, the reference
ramp's branches, PID saturation, the slip angles' singularity, every hold rule of the plant and the accept rule; and each C entry at
batch sizes off a multiple of its 64-thread block with a guard band behind every output.

Tolerance per tensor and table: max(32 e64, 1e-13 max(1, largest reference entry)), e64 the gap between the float64 and the long-double
run of the restatement over the table (frame_cases.tolerance; the rule of tests/test_exact_build_gpu.py) -- measured on the reference
alone.  finished, held cars and the take-over are compared exactly.  The heading error is compared on the circle (frame_cases.x0_error)
and must lie in [-pi, pi].  A case on whose discrete outcomes the two runs of the restatement disagree leaves the value comparisons
(tests/test_frame_cpu.py caps that at 2 % of a table and none of the named cases; today no case is dropped).  The measured errors are in
profiles/closed_loop_edges/README.md.

u_last of a held car: cl_plant_kernel returns before it writes anything, so a held car keeps the u_last it had."""
import ctypes as C

import numpy as np
import pytest

import frame_cases as fc
import frame_numpy as fn
import laps_numpy as lp

pytestmark = pytest.mark.gpu
LD = np.longdouble
GUARD = 512                       # doubles (or ints) behind every output of the batch-edge test
PATTERN = 0xA5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import fsae_mpc_amd as fm
    return fm, torch, fm.Track.load("fss2019"), fm.Track.from_points(*lp.circle_points(), M=lp.CIRCLE["M"])


def _dev(torch, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _groups(env):
    """[(track, target speed, [(table name, cases)])]: the tables of one track run as one batch"""
    _, _, track, circle = env
    return [(track, fc.TARGET_VEL, list(fc.frame_tables(track).items())), (circle, lp.CIRCLE["target_vel"], [("circle", fc.circle_table(circle)[0])])]


def _run_pre(env, model, N, track, tv, cases, reference=None, finished=None):
    fm, torch, _, _ = env
    cl = fm.ClosedLoop(model, N, fc.DT, track, np.array([c.cart for c in cases]), target_vel=tv, reference=reference)
    cl.x_opt[:, 0, 0] = _dev(torch, np.array([c.guess for c in cases]))
    if finished is not None:
        cl.finished.copy_(_dev(torch, finished, np.int32))
    cl.pre()
    torch.cuda.synchronize()
    return cl.x0.cpu().numpy(), cl.x_ref.cpu().numpy(), cl.finished.cpu().numpy()


def _check_frame(what, model, N, track, tv, tables, x0, x_ref, fin, with_x_ref=True):
    """the slices of one batch against their tables' references; prints each tensor's error as a fraction of its tolerance"""
    at = 0
    for name, cases in tables:
        sl = slice(at, at + len(cases)); at += len(cases)
        ref = fc.frame_reference(track, cases, model, N, tv)
        keep = ~ref["dropped"]
        assert np.isfinite(x0[sl]).all() and (not with_x_ref or np.isfinite(x_ref[sl]).all()), (what, name)
        kept = [c for c, k in zip(cases, keep) if k]
        assert np.array_equal(fin[sl][keep], ref["finished"][keep]), (what, name, fin[sl].tolist(), ref["finished"].tolist())
        lost = ref["finished"] == 2
        assert (x0[sl][lost & keep] == 0).all(), (what, name)
        assert (np.abs(x0[sl][:, 2]) <= np.pi).all(), (what, name)
        e0 = fc.x0_error(x0[sl], ref["x0"])[keep].astype(np.float64)
        worst = [("x0", float(e0.max()), ref["tol"]["x0"], kept[int(np.argmax(e0.max(axis=1)))].name)]
        if with_x_ref:
            e1 = np.abs(x_ref[sl].astype(LD) - ref["x_ref"])[keep].astype(np.float64)
            worst.append(("x_ref", float(e1.max()), ref["tol"]["x_ref"], kept[int(np.argmax(e1.reshape(len(e1), -1).max(axis=1)))].name))
        for tensor, err, tol, at_case in worst:
            print("%-8s %-9s model %d N %2d %-5s err %.2e  e64 %.2e  tol %.2e  err/tol %.3f  (%s)  dropped %d of %d"
                  % (what, name, model, N, tensor, err, ref["e64"][tensor], tol, err / tol, at_case, int(ref["dropped"].sum()), len(cases)))
        for tensor, err, tol, at_case in worst:
            assert err <= tol, (what, name, tensor, err, tol, at_case)


@pytest.mark.parametrize("N", [3, 40])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_frame_values(env, model, N):
    """ClosedLoop.pre() on every frame table: x0 and x_ref per tensor, finished exactly, a lost car's x0 exactly zero."""
    for track, tv, tables in _groups(env):
        cases = [c for _, cs in tables for c in cs]
        x0, x_ref, fin = _run_pre(env, model, N, track, tv, cases)
        _check_frame("pre", model, N, track, tv, tables, x0, x_ref, fin)


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_finished_is_sticky(env, model):
    """pre() only ever raises the flag: a car marked 1 that is put back before the line stays 1 (its x0 is the transform of where it
    is now), a car marked 2 that is back on the track stays 2, and a car marked 1 that is lost now becomes 2."""
    fm, torch, track, _ = env
    lap = fc.frame_tables(track)["lap"]
    _, _, first = _run_pre(env, model, 3, track, fc.TARGET_VEL, lap)
    assert first.tolist() == [0, 1, 1, 0, 1, 0, 1]
    back = [fc.Case(fc.on_track(track, track.L - 5.0 - i, 0.1), track.L - 5.3 - i, "put back %d" % i) for i in range(len(lap))]
    x0, x_ref, second = _run_pre(env, model, 3, track, fc.TARGET_VEL, back, finished=first)
    assert second.tolist() == first.tolist()
    ref = fc.frame_reference(track, back, model, 3, fc.TARGET_VEL)
    assert (ref["finished"] == 0).all() and not ref["dropped"].any()
    assert float(fc.x0_error(x0, ref["x0"]).max()) <= ref["tol"]["x0"] and float(np.abs(x_ref.astype(LD) - ref["x_ref"]).max()) <= ref["tol"]["x_ref"]
    _, _, third = _run_pre(env, model, 3, track, fc.TARGET_VEL, back, finished=np.full(len(back), 2))
    assert (third == 2).all()
    lost = fc.frame_tables(track)["lost"][:4]                     # n = 2.999, 3.001, -2.999, -3.001
    _, _, fourth = _run_pre(env, model, 3, track, fc.TARGET_VEL, lost, finished=np.ones(4))
    assert fourth.tolist() == [1, 2, 1, 2]


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_plan_tracking_pre_step(env, model):
    """cl_pre_plan_kernel (a ClosedLoop with a reference plan) on the same tables: x0 and finished to the same restatement at the same
    tolerance (not bit for bit with cl_pre: the two kernels may contract their products differently).  Its x_ref is the plan's walk,
    which tests/test_plan_gpu.py holds to the oracle."""
    fm, torch, _, _ = env
    for track, tv, tables in _groups(env):
        plan = fm.Plan.profile(model, track, N_s=97)
        cases = [c for _, cs in tables for c in cs]
        x0, x_ref, fin = _run_pre(env, model, 3, track, tv, cases, reference=plan)
        _check_frame("pre_plan", model, 3, track, tv, tables, x0, x_ref, fin, with_x_ref=False)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("flags", ["flags", "null"])
@pytest.mark.parametrize("blocks", ["fixed", "blocks"])
@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_plant_values(env, model, blocks, flags):
    """ClosedLoop.plant() on every plant table, with the compiled-in constants and with one parameter block per car (block 0 is the
    default block: its cars are held to the same reference as on the fixed path), with a flag array and without one: cart, pid and
    u_last per tensor; a held car bit for bit what it was, u_last included; a non-finite reference entry non-finite, and the next
    pre() marks that car 2."""
    fm, torch, track, _ = env
    tables = list(fc.plant_tables().items())
    cases = [c for _, cs in tables for c in cs]
    B, N = len(cases), 3
    P = fc.param_blocks() if blocks == "blocks" else None
    cart0, pid0 = np.array([c.cart for c in cases]), np.array([c.pid for c in cases])
    cl = fm.ClosedLoop(model, N, fc.DT, track, cart0, plant_params=None if P is None else P[[c.block for c in cases]])
    cl.pid.copy_(_dev(torch, pid0))
    cl.finished.copy_(_dev(torch, [c.finished for c in cases], np.int32))
    u0 = np.tile(fc.U_LAST_BEFORE, (B, 1))
    cl.u_last.copy_(_dev(torch, u0))
    plan = np.zeros((B, N, cl.nx))
    plan[:, 0, 3] = [c.v_ref for c in cases]; plan[:, 0, cl.nx - 1] = [c.delta_ref for c in cases]
    plan[:, 1:, :] = 77.0                                          # (only the first stage is read)
    cl.x_opt = _dev(torch, plan)
    cl.plant(None if flags == "null" else _dev(torch, [c.exitflag for c in cases], np.int32))
    torch.cuda.synchronize()
    got = dict(cart=cl.cart.cpu().numpy(), pid=cl.pid.cpu().numpy(), u_last=cl.u_last.cpu().numpy())
    before = dict(cart=cart0, pid=pid0, u_last=u0)
    cl.finished.zero_()
    cl.pre()
    torch.cuda.synchronize()
    fin_after = cl.finished.cpu().numpy()
    at = 0
    for name, cs in tables:
        sl = slice(at, at + len(cs)); at += len(cs)
        ref = fc.plant_reference(cs, P, null_flags=flags == "null")
        keep, held = ~ref["dropped"], ref["held"]
        assert not (~held & (got["pid"][sl] == before["pid"][sl]).all(axis=1)).any(), (name, "a driving car was held")
        for k in ("cart", "pid", "u_last"):
            assert np.array_equal(_bits(got[k][sl][held]), _bits(before[k][sl][held])), (name, k, "a held car was written")
            assert fc.same_finite_pattern(got[k][sl][keep], ref[k][keep]), (name, k)
            err = fc.finite_error(got[k][sl][keep], ref[k][keep])
            print("plant    %-9s model %d %-6s %-5s %-6s err %.2e  e64 %.2e  tol %.2e  err/tol %.3f  dropped %d of %d"
                  % (name, model, blocks, flags, k, err, ref["e64"][k], ref["tol"][k], err / ref["tol"][k], int(ref["dropped"].sum()), len(cs)))
            assert err <= ref["tol"][k], (name, k, err, ref["tol"][k])
        blown = ~np.isfinite(ref["cart"].astype(np.float64)).all(axis=1)
        assert (fin_after[sl][blown] == 2).all(), (name, fin_after[sl].tolist())
        if name == "slip":
            assert blown.tolist() == [False, False, True, False]


@pytest.mark.parametrize("model,N", [(0, 3), (1, 9)], ids=["kinematic-N3", "dynamic-N9"])
def test_accept(env, model, N):
    """fsaempc_cl_accept_batch_device on the accept table, with the flag array and with a null pointer: bit for bit frame_numpy.accept
    (the kernel is copies and compares)."""
    fm, torch, _, _ = env
    nx = 5 if model == 0 else 7
    t = fc.accept_table(nx, N)
    B = len(t["name"])
    for with_flags in (True, False):
        x_new, u_new, x_keep, u_keep = (_dev(torch, t[k]) for k in ("x_new", "u_new", "x_keep", "u_keep"))
        flag = _dev(torch, t["exitflag"]) if with_flags else None
        rc = fm.lib().fsaempc_cl_accept_batch_device(model, N, B, _p(x_new), _p(u_new), _p(flag), _p(x_keep), _p(u_keep), None)
        torch.cuda.synchronize()
        assert rc == 0, fm.lib().fsaempc_last_error()
        xk, uk = x_keep.cpu().numpy(), u_keep.cpu().numpy()
        taken = 0
        for b in range(B):
            wx, wu = fn.accept(t["x_new"][b], t["u_new"][b], int(t["exitflag"][b]) if with_flags else None, t["x_keep"][b], t["u_keep"][b])
            assert np.array_equal(_bits(xk[b]), _bits(wx)) and np.array_equal(_bits(uk[b]), _bits(wu)), (t["name"][b], with_flags)
            taken += np.array_equal(wx, t["x_new"][b])
        assert taken == (2 if with_flags else 7)
        assert np.array_equal(_bits(x_new.cpu().numpy()), _bits(t["x_new"])) and np.array_equal(_bits(u_new.cpu().numpy()), _bits(t["u_new"]))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _banded(torch, rows, width, dtype, init=None):
    """a buffer of rows * width entries and GUARD more behind them, every byte PATTERN; the first part takes `init` if given"""
    size = 8 if dtype == torch.float64 else 4
    raw = torch.full(((rows * width + GUARD) * size,), PATTERN, dtype=torch.uint8, device="cuda:0")
    t = raw.view(dtype)
    if init is not None:
        t[: rows * width] = _dev(torch, init, np.float64 if dtype == torch.float64 else np.int32).reshape(-1)
    return raw, t


def _intact(raw, rows, width, size):
    return bool((raw[rows * width * size:] == PATTERN).all())


@pytest.mark.parametrize("model", [0, 1], ids=["kinematic", "dynamic"])
def test_batch_edges_and_stray_writes(env, model):
    """The three C entries (the plant with and without parameter blocks) at B = 1, 63, 64, 65 and 129 -- off and on a multiple of the
    64-thread block -- with a band of 0xA5 bytes behind the B rows of every output: the band is bit for bit intact, rows 0 .. B - 1
    are the bits the same cars get at B = 129, and B = 0 returns success and touches nothing."""
    fm, torch, track, _ = env
    L = fm.lib()
    nx, N, B_MAX = (5 if model == 0 else 7), 3, 129
    frame = [c for cs in fc.frame_tables(track).values() for c in cs]
    plant = [c for cs in fc.plant_tables().values() for c in cs]
    frame = [frame[i % len(frame)] for i in range(B_MAX)]
    plant = [plant[i % len(plant)] for i in range(B_MAX)]
    acc = fc.accept_table(nx, N)
    rows = lambda a: np.array([a[i % len(a)] for i in range(B_MAX)])
    blocks = fc.param_blocks()[[c.block for c in plant]]
    plan = np.zeros((B_MAX, N, nx)); plan[:, 0, 3] = [c.v_ref for c in plant]; plan[:, 0, nx - 1] = [c.delta_ref for c in plant]
    xP, yP = track.device(torch.device("cuda:0"))
    sp = fm._lib.Spline(track.M, track.dl, _p(xP), _p(yP))
    f64, i32 = torch.float64, torch.int32

    def run(B):
        n = max(B, 1)              # (B = 0 passes real pointers to one row: nothing may be touched)
        out, bands = {}, []

        def banded(name, width, dtype, init=None):
            raw, t = _banded(torch, n if B else 0, width, dtype, None if (init is None or B == 0) else init[:n])
            bands.append((name, raw, n if B else 0, width, 8 if dtype == f64 else 4))
            out[name] = t
            return _p(t)
        cart = _dev(torch, np.array([c.cart for c in frame[:n]])); guess = _dev(torch, np.array([c.guess for c in frame[:n]]))
        rc = L.fsaempc_cl_pre_batch_device(model, N, C.c_double(fc.DT), C.c_double(fc.TARGET_VEL), C.c_double(track.L), C.byref(sp), _p(cart), _p(guess), B,
                                           banded("x0", nx, f64), banded("x_ref", nx * N, f64), banded("finished", 1, i32, np.zeros(n)), None)
        assert rc == 0, L.fsaempc_last_error()
        for tag, par in (("", None), ("_p", fm._lib.ParamBlock(blocks[:n], n, "cuda:0"))):
            x_opt = _dev(torch, plan[:n]); fin = _dev(torch, [c.finished for c in plant[:n]], np.int32); flag = _dev(torch, [c.exitflag for c in plant[:n]], np.int32)
            rc = L.fsaempc_cl_plant_batch_device_p(model, N, C.c_double(fc.DT), B, par.ref() if par is not None else None,
                                                   banded("cart" + tag, 7, f64, np.array([c.cart for c in plant])), banded("pid" + tag, 4, f64, np.array([c.pid for c in plant])),
                                                   _p(x_opt), _p(fin), _p(flag), banded("u_last" + tag, 2, f64, np.tile(fc.U_LAST_BEFORE, (B_MAX, 1))), None)
            assert rc == 0, L.fsaempc_last_error()
        x_new, u_new, flag = _dev(torch, rows(acc["x_new"])[:n]), _dev(torch, rows(acc["u_new"])[:n]), _dev(torch, rows(acc["exitflag"])[:n], np.int32)
        rc = L.fsaempc_cl_accept_batch_device(model, N, B, _p(x_new), _p(u_new), _p(flag), banded("x_keep", nx * N, f64, rows(acc["x_keep"])),
                                              banded("u_keep", 2 * N, f64, rows(acc["u_keep"])), None)
        assert rc == 0, L.fsaempc_last_error()
        torch.cuda.synchronize()
        for name, raw, r, width, size in bands:
            assert _intact(raw, r, width, size), (B, name, "a write behind the batch's rows")
        return {k: v[: (n if B else 0) * w].cpu().numpy() for (k, _, _, w, _), v in zip(bands, out.values())}

    full = run(B_MAX)
    assert (full["finished"] != 0).any() and (full["finished"] == 0).any()
    for B in (1, 63, 64, 65):
        part = run(B)
        for k, v in part.items():
            assert np.array_equal(_bits(v), _bits(full[k][: v.size])), (B, k)
    run(0)
