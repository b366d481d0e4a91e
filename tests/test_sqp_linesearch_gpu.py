"""GPU tests of csrc/sqp.hip against tests/sqp_numpy.py, sweep by sweep.  SqpBatch.solve is deterministic, so its state
after max_sweeps = k is the state of a longer run after sweep k: for k = 1 .. 5 the test takes the instances still running after sweep
k - 1, replays the sweep's QP on the device through the public API (build_qp, qp_solve_batch_device with the batch's options and x_init =
(u, s)), asserts that the replayed multipliers are bit for bit those the sweep returned (so the replayed z is the z the kernel saw), runs
sqp_numpy.sweep on that QP and requires the device's result to be one of the admissible outcomes.  The init kernel is seen through a run
whose Armijo constant (1e30) rejects every trial: such an instance returns its start.  A last test runs the compaction kernel with more
than one instance per thread and holes in the running set."""
import numpy as np
import pytest

import sqp_cases as sc
import sqp_numpy as sq

pytestmark = pytest.mark.gpu

DT = sc.DT
KEYS = ("u_opt", "x_opt", "slack", "fval", "status", "sweeps", "qp_iter", "merit")      # as test_sqp_instances_are_isolated


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
def tracks(fm, orc):
    return fm.Track.load("fsg2019"), orc.Track.load(fm.tracks._HERE + "/tracks/fsg2019.json")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _solve(sb, torch, x0, xr, u, **kw):
    out = sb.solve(_dev(torch, x0), _dev(torch, xr), _dev(torch, u), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _close(a, b, tol):
    """|a - b| <= tol max(1, |b|), entry by entry."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b)))))


def _point_diffs(out, b, u, s, X, J, vmax):
    """Names of the outputs of instance b that are not the point (u, s, X, J, vmax) within the tolerances: u 1e-14 max(1, |u|) (the same
    arithmetic up to a fused multiply-add), x_opt 1e-10 relative (the suite's rollout tolerance), slack 1e-10 max(1, |s|), fval 1e-9
    relative (the suite's objective tolerance), hard_viol 1e-10 max(1, |X|) (a difference of rollout states)."""
    bad = []
    if not _close(out["u_opt"][b], np.ravel(u), 1e-14): bad.append("u_opt")
    if not _rel(out["x_opt"][b], np.ravel(X)) <= 1e-10: bad.append("x_opt")
    if not _close(out["slack"][b], s, 1e-10): bad.append("slack")
    if not _close(out["fval"][b], J, 1e-9): bad.append("fval")
    if not abs(out["hard_viol"][b] - vmax) <= 1e-10 * max(1.0, float(np.max(np.abs(X)))): bad.append("hard_viol")
    return bad


def _outcome_diffs(out, b, k, r, oc):
    bad = _point_diffs(out, b, oc["u"], oc["s"], oc["X"], oc["J"], oc["vmax"])
    if out["status"][b] != oc["status"]: bad.append("status")
    if out["sweeps"][b] != oc["sweeps"]: bad.append("sweeps")
    if not _close(out["merit"][b, k - 1], oc["merit"], 1e-9): bad.append("merit")
    if not abs(out["step_norm"][b] - r["step_norm"]) <= 1e-14 * abs(r["step_norm"]): bad.append("step_norm")
    return bad


_DONE = {}


def _replayed(fm, torch, orc, tracks, name):
    """The replay of one case, with all its assertions, run once: dict(records, ambiguous, total)."""
    if name not in _DONE:
        try:
            _DONE[name] = _replay(fm, torch, orc, tracks, name)
        except BaseException as e:      # (the coverage test meets the same failure without running the case again)
            _DONE[name] = e
    if isinstance(_DONE[name], BaseException):
        raise _DONE[name]
    return _DONE[name]


def _replay(fm, torch, orc, tracks, name):
    import nlp_numpy as nn
    tr, otr = tracks
    model, N, x0, xr, u_init = sc.inputs(fm, tr.L, name)
    o = sc.options(name)
    B = x0.shape[0]
    nx, ns, nV, nC = fm.dims(model, N)
    Ps = [sq.Problem(orc, model, otr, x0[b], xr[b], DT, nn.default_integrator(model)) for b in range(B)]
    sb = fm.SqpBatch(model, N, DT, tr, B)
    outs = {k: _solve(sb, torch, x0, xr, u_init, max_sweeps=k, **o) for k in range(1, sc.SWEEPS + 1)}

    # 1. every returned point is a point of the NLP, and the merit entries beyond `sweeps` are NaN
    for k, out in outs.items():
        assert out["merit"].shape == (B, k)
        for b in range(B):
            if out["status"][b] < 0 and not np.all(np.isfinite(out["x_opt"][b])):
                continue
            e = sq.evaluate(Ps[b], out["u_opt"][b], out["u_opt"][b], 0.0, out["slack"][b])
            assert np.array_equal(e.u.ravel(), out["u_opt"][b]), (name, k, b)      # inside the boxes (e.s = max(slack, s_min): compared below)
            assert not _point_diffs(out, b, e.u, e.s, e.X, e.J, e.vmax), (name, k, b, _point_diffs(out, b, e.u, e.s, e.X, e.J, e.vmax))
            n = out["sweeps"][b]
            assert 1 <= n <= k and np.all(np.isnan(out["merit"][b, n:])) and np.all(np.isfinite(out["merit"][b, :n])), (name, k, b, out["merit"][b])

    # the init kernel: with armijo = 1e30 no trial of a sweep with pred > 0 is accepted, so the instance returns its start
    init = [sq.evaluate(Ps[b], u_init[b], u_init[b], 0.0, np.zeros(ns)) for b in range(B)]
    probe = _solve(sb, torch, x0, xr, u_init, max_sweeps=1, **dict(o, armijo=1e30))
    held = np.isin(probe["status"], (2, -1, -2))
    assert held.sum() >= B // 2, (name, probe["status"])
    u_prev = np.stack([e.u.ravel() for e in init])
    s_prev = np.stack([e.s for e in init])
    for b in np.flatnonzero(held):
        bad = _point_diffs(probe, b, init[b].u, init[b].s, init[b].X, init[b].J, init[b].vmax)
        assert not bad and np.array_equal(probe["u_opt"][b], init[b].u.ravel()), (name, "init", b, bad)       # the clip is exact
        s_prev[b] = probe["slack"][b]                     # the device's own bits: the replayed QP starts from them
    clipped = np.any(u_prev != u_init.reshape(B, -1), axis=1)

    rho = np.full(B, float(o["rho0"]))
    prev = None
    records, amb = [], 0
    for k in range(1, sc.SWEEPS + 1):
        out = outs[k]
        ran = np.arange(B) if prev is None else np.flatnonzero((prev["status"] == 1) & (prev["sweeps"] == k - 1))
        if prev is not None:
            rest = np.setdiff1d(np.arange(B), ran)          # ended before sweep k: nothing of theirs moves
            assert np.all(prev["status"][rest] != 1)
            for key in KEYS + ("lambda", "step_norm", "hard_viol"):
                a, p = out[key][rest], prev[key][rest]
                if key == "merit":
                    assert np.all(np.isnan(a[:, k - 1])), (name, k)
                    a = a[:, :k - 1]
                assert np.array_equal(a, p, equal_nan=True), (name, k, key)
            u_prev, s_prev = prev["u_opt"], prev["slack"]
        if ran.size == 0:
            break
        # 2. the sweep's QP again, through the public API
        sbk = sb if ran.size == B else fm.SqpBatch(model, N, DT, tr, int(ran.size))
        q = sbk.build_qp(_dev(torch, x0[ran]), _dev(torch, xr[ran]), _dev(torch, u_prev[ran]))
        xin = _dev(torch, np.concatenate([u_prev[ran], s_prev[ran]], axis=1)) if o["warm_start"] else None
        r = fm.qp_solve_batch_device(q["H"], q["g"], q["A"], q["lb"], q["ub"], q["lbA"], q["ubA"], options=sbk.opts, want_lambda=True, x_init=xin)
        torch.cuda.synchronize()
        z, fq, fl, it, lam, qc = (t.cpu().numpy() for t in (r["x"], r["fval"], r["exitflag"], r["iter"], r["lam"], q["const"]))
        # link: the multipliers the sweep returned are the replay's, bit for bit, and its iterations are the increase of qp_iter
        assert np.array_equal(out["lambda"][ran], lam, equal_nan=True), (name, k, "lambda of the replayed QP differs from the sweep's")
        base = 0 if prev is None else prev["qp_iter"][ran]
        assert np.array_equal(out["qp_iter"][ran] - base, it), (name, k, out["qp_iter"][ran], base, it)
        # 3. the line search
        for j, b in enumerate(ran):
            here = sq.evaluate(Ps[b], u_prev[b], u_prev[b], 0.0, s_prev[b])
            res = sq.sweep((u_prev[b], s_prev[b], rho[b], here.J, here.viol), sq.Qp(z[j], float(fq[j]), float(qc[j]), int(fl[j]), int(it[j]), lam[j]),
                           sq.Opts(o["trials"], o["armijo"], o["tol_step"], o["tol_feas"], k - 1, k), Ps[b])
            rho[b] = res["rho"]
            diffs = {l: _outcome_diffs(out, b, k, res, res["outcomes"][l]) for l in res["admissible"]}
            match = [l for l in res["admissible"] if not diffs[l]]
            assert match, (name, "sweep", k, "instance", b, "admissible", res["admissible"], "differences", diffs, "margins", res["margins"],
                           "tau", res["tau"], "status", out["status"][b], "step_norm", out["step_norm"][b], res["step_norm"])
            amb += len(res["admissible"]) > 1
            oc = res["outcomes"][match[0]]
            records.append(dict(winner=match[0], status=sq.RUNNING if out["status"][b] == 1 else int(out["status"][b]),
                                viol_start=here.viol, clipped=bool(clipped[b]) and k == 1, lam_hard=float(np.max(np.abs(lam[j][nV:nV + 2 * N]))),
                                rho_seen=res["rho"] * oc["viol"] > 1e-7 * max(1.0, abs(oc["merit"]))))
        prev = out
    # 4. few enough decisions within the tolerance
    assert amb <= sc.CAP * len(records), (name, amb, len(records))
    return dict(records=records, ambiguous=amb, total=len(records))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_sweeps_match_the_restatement(fm, torch_, orc, tracks, name):
    """Every sweep of every instance of the case gives one admissible outcome of sqp_numpy.sweep on the sweep's own QP; the share of
    instance-sweeps with more than one admissible outcome is at most a third."""
    got = _replayed(fm, torch_, orc, tracks, name)
    c = sc.coverage(got["records"])
    print("%s: %d of %d instance-sweeps with more than one admissible outcome; %s; largest multiplier of a hard row %.3g"
          % (name, got["ambiguous"], got["total"], c, max(r["lam_hard"] for r in got["records"])))


def test_device_sweeps_exercise_every_path(fm, torch_, orc, tracks):
    """What the device actually did over all cases: full steps, backtracked steps, status 2, status 0, sweeps that start with a hard
    violation, clipped starts; and in the case made for it, active hard rows whose rho is visible in the merit."""
    recs = {name: _replayed(fm, torch_, orc, tracks, name)["records"] for name in sc.CASES}
    c = sc.coverage(r for v in recs.values() for r in v)
    assert all(c[k] >= 1 for k in ("full", "backtrack", "status2", "status0", "viol", "clipped")), c
    a = sc.coverage(recs[sc.ACTIVE])
    assert a["lam_hard_viol"] >= 1 and sum(r["rho_seen"] and r["lam_hard"] > 0 for r in recs[sc.ACTIVE]) >= 1, a


def _picks(B):
    """16 instances of a batch of B with every 7th x0 NaN (i % 7 == 5): the first, the last, both neighbours of the two chunk boundaries of
    sqp_compact_kernel next to B / 2, NaN instances with their neighbours, the rest evenly spread."""
    chunk = (B + 1023) // 1024
    c0 = (B // 2) // chunk * chunk
    p = [0, B - 1, c0 - 1, c0, c0 + chunk - 1, c0 + chunk]
    for at in (B // 4, 3 * B // 4):
        j = at // 7 * 7 + 5
        p += [j - 1, j, j + 1]
    for i in np.linspace(1, B - 2, 40).astype(int):
        if len(set(p)) >= 16:
            break
        p.append(int(i))
    p = sorted(set(p))
    assert len(p) == 16 and p[0] == 0 and p[-1] == B - 1
    return p


@pytest.mark.parametrize("B", [1024, 1025, 2049, 3000])
def test_compaction_with_chunks_and_holes(fm, torch_, tracks, B):
    """sqp_compact_kernel gives each of its 1024 threads ceil(B / 1024) instances: one (B = 1024, the last size that does), two, three with
    a ragged end.  Every 7th instance has a NaN x0 and leaves at the first sweep (status -1), so the later sweeps compact a running set
    with holes across the chunk boundaries; 16 instances agree bit for bit with their solo solves."""
    torch = torch_
    tr, _ = tracks
    model, N = 0, 5
    x0, _, ul, xr = fm.instances(model, N, DT, tr.L, sc.SEED, range(B))
    nan = np.arange(B) % 7 == 5
    x0[nan] = np.nan
    full = _solve(fm.SqpBatch(model, N, DT, tr, B), torch, x0, xr, ul, max_sweeps=3)
    assert np.all(full["status"][nan] == -1), np.unique(full["status"][nan], return_counts=True)
    assert np.all(full["sweeps"][nan] == 1)
    assert np.all(np.isin(full["status"][~nan], (0, 1, 2, -1, -2))) and np.sum(full["status"][~nan] == 1) >= B // 2   # (most run all three sweeps)
    one = fm.SqpBatch(model, N, DT, tr, 1)
    for b in _picks(B):
        solo = _solve(one, torch, x0[b:b + 1], xr[b:b + 1], ul[b:b + 1], max_sweeps=3)
        for k in KEYS:
            assert np.array_equal(solo[k][0], full[k][b], equal_nan=True), (B, b, k, solo[k][0], full[k][b])
