"""The case table of the SQP line-search tests, shared by tests/test_sqp_linesearch_cpu.py (which vets every case with the
all-CPU loop of tests/sqp_numpy.py) and tests/test_sqp_linesearch_gpu.py (which replays the device's sweeps against sqp_numpy.sweep).
fsg2019, dt 0.05, synthetic seed 31, B = 12 instances per case: the smallest shapes at which sqp.hip takes each of its paths.

Two remarks on the starts.  (1) fm.instances returns u_lin = 0, so "a multiple of u_lin" cannot leave the input box: the clipped start is
written out below (|a| up to 12, |steer rate| up to 0.6).  (2) The multipliers of the hard rows are exactly zero in the natural cases and
in the violating starts at ids 0 .. 11, so rho never moves there; the case ACTIVE has them active (_steer_demand)."""
import numpy as np

import sqp_numpy as sq

DT = 0.05
SEED = 31
B = 12
SWEEPS = 5          # replayed sweeps: the ambiguous decisions concentrate in the converged tail, where pred -> 0
CAP = 1.0 / 3.0     # largest admitted share of instance-sweeps with more than one admissible outcome, per case


def _plain(x0, u):
    return x0, u


def _steer_start(x0, u):
    """delta_0 = 0.395 and the steer rate at its bound: delta_k = 0.395 + 0.02 k, l1 violation of |delta_k| <= 0.4: 1.05 at N = 10."""
    x0 = x0.copy(); u = u.copy()
    x0[:, -1] = 0.395
    u[:, :, 1] = 0.4
    return x0, u


def _brake_start(x0, u):
    """v_0 = 0.3 and full braking: v_k = 0.3 - 0.5 k, l1 violation of v_k >= 0: 24.5 at N = 10."""
    x0 = x0.copy(); u = u.copy()
    x0[:, 3] = 0.3
    u[:, :, 0] = -10.0
    return x0, u


def _outside_box(x0, u):
    """Every entry outside or inside the box by turns: a = 12 cos(k + b), steer rate = 0.6 sin(2 k + b); init must clip it."""
    u = u.copy()
    k, b = np.arange(u.shape[1])[None, :], np.arange(u.shape[0])[:, None]
    u[:, :, 0] = 12.0 * np.cos(k + b)
    u[:, :, 1] = 0.6 * np.sin(2 * k + b)
    return x0, u


def _steer_demand(x0, u):
    """A start on the steering limit whose reference asks for more: slow (v_0 = 3, so the lateral-acceleration row stays slack), delta_0 =
    0.395 with the steer rate at its bound (the start violates |delta_k| <= 0.4), and x_ref n half a metre towards the turn, so that the
    QP's rows delta_k <= 0.4 are active: their multipliers are not zero and rho rises above rho0."""
    x0, u = _steer_start(x0, u)
    x0[:, 3] = 3.0
    return x0, u


def _steer_demand_ref(x0, xr):
    xr = xr.copy()
    xr[:, :, 1] = x0[:, None, 1] + 0.5
    xr[:, :, 2] = 0.3
    return xr


# The ids of the steering-limit start.  At delta = 0.4 and v_0 >= 5 the lateral-acceleration row needs a slack of 1.7 .. 100, which at its
# cost of 1e8 puts J at 2e8 .. 8e9: the admitted band of an Armijo decision, 1e-8 (1 + |phi0|), is then 2 .. 80 wide in absolute terms, and
# from the second or third sweep on pred is below it.  With ids 0 .. 11 the all-CPU loop has 36 of 57 instance-sweeps with more than one
# admissible outcome, and of the ids 0 .. 1499 only nine stay at or below a third on their own (102, 416, 507, 636, 704, 711, 755, 828,
# 1201: slow ones, whose pred stays large); 13, 16 and 20 (two of four each) complete the dozen.  Sweep 0, the one these cases are for
# (rho viol in phi0 and pred), is unambiguous for every id.
STEER_IDS = (13, 16, 20, 102, 416, 507, 636, 704, 711, 755, 828, 1201)

# name: (model, N, ids, SQP options, start, reference edit or None)
CASES = {
    # shapes
    "kin10": (0, 10, range(B), {}, _plain, None),                                  # the plain case
    "kin40": (0, 40, range(B), {}, _plain, None),                                  # 2N = 80 > 64: the lane-strided maxima make a second pass
    "dyn12": (1, 12, range(B), {}, _plain, None),                                  # four slacks, slip and 12-gon rows in the reset, RK4
    # option edges
    "trials1": (0, 10, range(B), dict(trials=1), _plain, None),                    # full step or status 2
    "trials64": (0, 10, range(B), dict(trials=64), _plain, None),                  # every lane evaluates, alpha down to 2^-63
    "armijo0.9": (0, 10, range(B), dict(armijo=0.9), _plain, None),                # backtracking
    "rho0": (0, 10, range(B), dict(rho0=0.0), _plain, None),
    "rho1000": (0, 10, range(B), dict(rho0=1000.0), _plain, None),
    "cold": (0, 10, range(B), dict(warm_start=0), _plain, None),
    # starts that violate the hard rows: rho viol enters phi0 and pred at sweep 0
    "steer_rho1": (0, 10, STEER_IDS, dict(rho0=1.0), _steer_start, None),
    "steer_rho1000": (0, 10, STEER_IDS, dict(rho0=1000.0), _steer_start, None),
    "brake_rho1": (0, 10, range(B), dict(rho0=1.0), _brake_start, None),
    "brake_rho1000": (0, 10, range(B), dict(rho0=1000.0), _brake_start, None),
    # a start outside the input box
    "outside_box": (0, 10, range(B), {}, _outside_box, None),
    # active hard rows: rho rises above rho0 = 0; armijo > 1 refuses the full step (a quadratic model gains (2 - alpha) alpha pred, so
    # alpha = 1/2 passes up to armijo = 1.5), and the accepted point keeps a violation: rho' viol stays visible in the merit entry
    "active": (0, 10, range(B), dict(rho0=0.0, armijo=1.2), _steer_demand, _steer_demand_ref),
}
ACTIVE = "active"

DEFAULTS = dict(trials=8, armijo=1e-4, tol_step=1e-6, tol_feas=1e-6, rho0=1.0, warm_start=1)


def options(name):
    """The SQP options of a case (without max_sweeps), defaults filled in: the keywords of SqpBatch.solve."""
    o = dict(DEFAULTS)
    o.update(CASES[name][3])
    return o


def inputs(fm, L, name):
    """model, N, x0 (B, nx), x_ref (B, N, nx), u_init (B, N, 2) of a case."""
    model, N, ids, _, start, ref = CASES[name]
    x0, _, ul, _ = fm.instances(model, N, DT, L, SEED, ids)
    x0, u = start(x0, ul)
    xr = fm.synthetic.reference_live(x0, N, DT, 20.0)       # (the reference of the start's own x0, as fm.instances makes it)
    if ref is not None:
        xr = ref(x0, xr)
    return model, N, x0, xr, u


def problems(orc, otr, fm, name):
    """One sqp_numpy.Problem per instance of a case, and its u_init."""
    import nlp_numpy as nn
    model, N, x0, xr, u = inputs(fm, otr.L, name)
    return [sq.Problem(orc, model, otr, x0[b], xr[b], DT, nn.default_integrator(model)) for b in range(x0.shape[0])], u


_C = {}


def cpu_runs(orc, otr, fm, name):
    """sqp_numpy.cpu_loop of every instance of a case over SWEEPS sweeps, computed once."""
    if name not in _C:
        o = options(name)
        Ps, u = problems(orc, otr, fm, name)
        _C[name] = [sq.cpu_loop(P, u[b], SWEEPS, trials=o["trials"], armijo=o["armijo"], tol_step=o["tol_step"], tol_feas=o["tol_feas"],
                                rho0=o["rho0"]) for b, P in enumerate(Ps)]
    return _C[name]


def coverage(records):
    """What a set of sweeps exercised.  records: iterable of dict(winner, status, viol_start, clipped, lam_hard) per instance-sweep."""
    c = dict(full=0, backtrack=0, status2=0, status0=0, qp_failed=0, viol=0, clipped=0, lam_hard=0, lam_hard_viol=0)
    for r in records:
        c["qp_failed"] += r["status"] < 0
        c["full"] += r["winner"] == 0
        c["backtrack"] += r["winner"] is not None and r["winner"] >= 1
        c["status2"] += r["status"] == 2
        c["status0"] += r["status"] == 0
        c["viol"] += r["viol_start"] > 0
        c["clipped"] += bool(r["clipped"])
        c["lam_hard"] += r["lam_hard"] > 0
        c["lam_hard_viol"] += r["lam_hard"] > 0 and r["viol_start"] > 0
    return c
