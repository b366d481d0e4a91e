"""CPU tests of the line-search restatement (tests/sqp_numpy.py) and of the case table (tests/sqp_cases.py) that
tests/test_sqp_linesearch_gpu.py replays on the device: the all-CPU loop (central-difference build, the oracle's QP solve,
sqp_numpy.sweep) obeys the rule's own invariants on every case, the table exercises what it is for, and few enough of its decisions
lie within the admitted tolerance of the Armijo test."""
import numpy as np
import pytest

import nlp_numpy as nn
import sqp_cases as sc
import sqp_numpy as sq


@pytest.fixture(scope="module")
def fm():
    import fsae_mpc_amd
    return fsae_mpc_amd


def _records(runs):
    for run in runs:
        for k, r in enumerate(run["records"]):
            out = r["outcomes"][r["winner"]]
            yield dict(winner=r["winner"], status=out["status"], viol_start=r["start"][1], clipped=run["clipped"] and k == 0,
                       lam_hard=r["lam_hard"], rho_seen=r["rho"] * out["viol"] > 1e-7 * max(1.0, abs(out["merit"])))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_cpu_loop_obeys_the_rule(orc, otrack, fm, name):
    """Per case: the merit never rises, every accepted iterate is inside the boxes with s >= s_min, the statuses follow the rule, and at
    most a third of the instance-sweeps have more than one admissible outcome."""
    o = sc.options(name)
    Ps, _ = sc.problems(orc, otrack, fm, name)
    runs = sc.cpu_runs(orc, otrack, fm, name)
    total = amb = 0
    for b, (P, run) in enumerate(zip(Ps, runs)):
        assert np.all(np.abs(run["init"].u) <= sq.U_MAX) and np.all(run["init"].s >= 0), b
        assert len(run["records"]) >= 1
        for k, r in enumerate(run["records"]):
            w = r["winner"]
            out = r["outcomes"][w]
            total += 1
            amb += len(r["admissible"]) > 1
            assert w in r["admissible"], (b, k)
            J0, viol0, s0 = r["start"]
            assert r["phi0"] == J0 + r["rho"] * viol0 and r["pred"] >= 0, (b, k)
            assert out["merit"] <= r["phi0"], (b, k, out["merit"], r["phi0"])
            assert np.all(np.abs(out["u"]) <= sq.U_MAX), (b, k)
            assert np.all(out["s"] >= nn.slack_min(P.model, out["X"], out["u"])) and np.all(out["s"] >= 0), (b, k)
            last = k + 1 == sc.SWEEPS
            if w is None:
                assert out["status"] in (0, 2, -1, -2) and np.array_equal(out["s"], s0), (b, k)
                assert np.all(~(r["margins"] >= 0)), (b, k)
                if out["status"] == 0:
                    assert r["step_norm"] <= o["tol_step"] * (1 + np.abs(out["u"]).max()) and out["vmax"] <= o["tol_feas"], (b, k)
            else:
                assert r["margins"][w] >= 0 and np.all(~(r["margins"][:w] >= 0)), (b, k)
                assert out["status"] in ((0, 1) if last else (0, sq.RUNNING)), (b, k)
                assert out["merit"] <= r["phi0"] - o["armijo"] * 2.0 ** -w * r["pred"], (b, k)
            if out["status"] != sq.RUNNING:
                assert k + 1 == len(run["records"]), (b, k)      # nothing runs after a final status
        assert run["status"] != sq.RUNNING, b
    assert amb <= sc.CAP * total, (name, amb, total)


def test_table_exercises_every_path(orc, otrack, fm):
    """Over all cases and their first five sweeps: a full step, a backtracked step, a status 2, a status 0, a sweep that starts with a
    hard violation and a clipped start all occur."""
    c = sc.coverage(r for name in sc.CASES for r in _records(sc.cpu_runs(orc, otrack, fm, name)))
    assert all(c[k] >= 1 for k in ("full", "backtrack", "status2", "status0", "viol", "clipped")), c
    # active hard rows: rho rises above rho0 = 0 in a sweep that starts with a violation, and an accepted point keeps a violation, so
    # that rho' viol is a visible part (100 times the merit's tolerance) of the merit entry the kernel writes
    act = list(_records(sc.cpu_runs(orc, otrack, fm, sc.ACTIVE)))
    assert sc.coverage(act)["lam_hard_viol"] >= 1 and sum(r["rho_seen"] and r["lam_hard"] > 0 for r in act) >= 1
    # what the issue's own CPU run saw: trials = 1 leaves some of ids 0, 1, 4, 5 at status 2; armijo = 0.9 backtracks
    st = [run["status"] for run in sc.cpu_runs(orc, otrack, fm, "trials1")]
    assert any(st[b] == 2 for b in (0, 1, 4, 5)), st
    assert any(r["winner"] not in (0, None) for run in sc.cpu_runs(orc, otrack, fm, "armijo0.9") for r in run["records"])
    for name, viol in (("steer_rho1", 1.05), ("brake_rho1", 24.5)):
        v = np.array([run["init"].viol for run in sc.cpu_runs(orc, otrack, fm, name)])
        assert np.all(np.abs(v - viol) <= 0.06 * viol), (name, v)      # (the brake start's delta_0 moves it a little, the rest is exact)


def test_admissible_set_on_hand_made_margins():
    A = sq.admissible
    assert A([1.0, 1.0], 0.1) == [0]                              # a clear full step
    assert A([-1.0, 1.0, 1.0], 0.1) == [1]                        # a clear backtrack: the lowest accepted trial
    assert A([-1.0, -1.0], 0.1) == [None]                         # all rejected
    assert A([], 0.1) == [None]                                   # no trial evaluated (a failed QP)
    assert A([0.05, 1.0], 0.1) == [0, 1]                          # the full step within tau of the threshold: it or the next
    assert A([-0.05, 1.0], 0.1) == [0, 1]
    assert A([-0.05, -1.0, 0.05], 0.1) == [0, 2, None]            # two ties around a clear rejection
    assert A([0.1, -1.0], 0.1) == [0, None]                       # a margin of exactly tau is still a tie ...
    assert A([-0.1, -1.0], 0.1) == [0, None]                      # ... on both sides
    assert A([0.1000001, -1.0], 0.1) == [0]
    assert A([-0.1000001, -1.0], 0.1) == [None]
    assert A([0.0, 0.0], 0.0) == [0, 1, None]                     # tau = 0: only exact ties are ambiguous
    nan = float("nan")
    assert A([nan, 1.0], 0.1) == [1]                              # a NaN trial is rejected, whatever tau
    assert A([nan, nan], 0.1) == [None]
    assert A([nan, 0.05, nan, 1.0], 0.1) == [1, 3]
    assert A([-1.0, 0.05, 0.05, -1.0], 0.1) == [1, 2, None]
