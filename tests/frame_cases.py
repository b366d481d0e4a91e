"""The case tables of tests/test_frame_cpu.py and tests/test_frame_gpu.py: cars at the edges of the frame transform, the plant and the
plan take-over, and what both files need of frame_numpy on them (frame_reference, plant_reference: both dtypes of the restatement, the
drop rule, e64 and the tolerance).  A frame table is a list of Case(cart (7,), guess, name); a plant table a list of PlantCase; the accept
table a dict of arrays.  Every table is small and named, and its tolerance is worked out from its own cars (tolerance()).  A track is
any object with xP, yP (M x 4), M, dl, L.

Speeds are chosen off the grid v + 0.5 k = target_vel (10 dt = 0.5 with dt = 0.05): on it the ramp reaches the target exactly and which
side of the clip a stage falls on is decided by the last bit of 10 * dt, with the same value either way."""
from collections import namedtuple

import numpy as np

import frame_numpy as fn
import lap_numpy as ln
import laps_numpy as lp
import param_numpy as pn
from dual_numpy import default_block

DT = 0.05
TARGET_VEL = 20.3          # (off the grid of every speed below; the circle table has its own)
V0 = 8.7                   # the speed of a car whose speed is not the point of its case
Case = namedtuple("Case", "cart guess name")
PlantCase = namedtuple("PlantCase", "cart pid v_ref delta_ref finished exitflag block name")


def tolerance(e64, ref):
    """max(32 e64, 1e-13 max(1, largest finite reference entry)): the rule of tests/test_exact_build_gpu.py over the table's batch"""
    ref = np.asarray(ref, dtype=np.float64)
    big = float(np.max(np.abs(ref[np.isfinite(ref)]))) if np.isfinite(ref).any() else 0.0
    return max(32.0 * float(e64), 1e-13 * max(1.0, big))


def on_track(track, s, n, v=V0, dtheta=0.0):
    """[x, y, theta, v, 0, 0, 0] at arc length s, lateral offset n, heading along the track plus dtheta (lap_numpy.cart_on_track)"""
    c = ln.cart_on_track(track, s, n, v)
    c[2] += dtheta
    return c


def kappa(track, s):
    _, xd, xdd = fn.spline3(track, track.xP, s, np.float64)
    _, yd, ydd = fn.spline3(track, track.yP, s, np.float64)
    return (xd * ydd - xdd * yd) / (xd * xd + yd * yd) ** 1.5


def random_carts(track, B, seed):
    """The draw of test_gpu_parity._random_carts: the first 90 % of the track, |n| <= 0.5 m, heading error <= 0.1 rad, speed 0 .. 25,
    a Newton guess within 1 m"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(B):
        s, n = rng.uniform(0, track.L * 0.9), rng.uniform(-0.5, 0.5)
        c = ln.cart_on_track(track, s, n, 0.0)
        c[2] += rng.uniform(-0.1, 0.1)
        c[3:] = [rng.uniform(0, 25), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1)]
        out.append(Case(c, s + rng.uniform(-1, 1), "random %d" % i))
    return out


def tightest_corner(track):
    s = np.arange(0.0, track.L, 0.25)
    k = np.array([kappa(track, v) for v in s])
    i = int(np.argmax(np.abs(k)))
    return float(s[i]), float(k[i])


def frame_tables(track):
    """name -> list of Case on `track` (fss2019 in the tests), target speed TARGET_VEL"""
    L, dl = track.L, track.dl
    T = {}
    T["ordinary"] = random_carts(track, 32, 3)
    # heading against the track
    s = 50.0
    T["heading"] = [Case(on_track(track, s, 0.2, dtheta=d), s, name) for d, name in     # (guess = s: the heading is taken where the car was put)
                    [(np.pi, "theta = heading + pi"), (-np.pi, "theta = heading - pi"), (np.pi - 1e-12, "theta = heading + (pi - 1e-12)"),
                     (-(np.pi - 1e-12), "theta = heading - (pi - 1e-12)"), (2 * np.pi, "theta + 2 pi"), (-2 * np.pi, "theta - 2 pi"),
                     (6 * np.pi, "theta + 6 pi"), (-6 * np.pi, "theta - 6 pi")]]
    # Newton search
    sc, kc = tightest_corner(track)
    k17 = 17 * dl
    T["newton"] = [
        Case(on_track(track, 60.0, 0.3), 65.0, "guess 5 m off"),
        Case(on_track(track, 60.0, 0.3), 40.0, "guess 20 m off"),
        Case(on_track(track, 20.0, 0.3), 20.0 + L / 2, "guess half a lap off"),         # (settles 33 m off the track: lost)
        Case(on_track(track, L - 10.0, -0.2), -10.5, "guess below 0"),
        Case(on_track(track, 10.0, -0.2), L + 10.5, "guess above L"),
        Case(on_track(track, k17 + 0.3, 0.1), k17, "guess on a segment boundary"),
        Case(on_track(track, k17, 0.1), k17, "car and guess on a segment boundary"),
        Case(on_track(track, sc, 1.5 / kc), sc + 2.5, "beyond the centre of curvature"),   # (walks 3 m on, ends 4.8 m off the track: lost)
        # a car 0.66 m off the centre line with a guess 25 m ahead: the search falls into a two-cycle around s = 256 and the guard ends it
        # (found by a random search on fss2019: 1.5 % of cars within 12 m of the line with a guess within 30 m never settle); lost
        Case(on_track(track, 231.88, -0.66), 256.64, "never settles: the 1000-step guard"),
    ]
    # lap check: the closest point just below, at and above L, and further out on both sides
    T["lap"] = [Case(on_track(track, v, 0.0), v, name) for v, name in
                [(L - 1e-9, "s = L - 1e-9"), (L, "s = L"), (L + 0.3, "s = L + 0.3"), (L - 0.3, "s = L - 0.3"), (L + 1e-9, "s = L + 1e-9")]]
    T["lap"] += [Case(on_track(track, L - 0.2, 0.3), L - 0.6, "s = L - 0.2 from a guess 0.4 m back"),
                 Case(on_track(track, L + 0.2, 0.3), L - 0.2, "s = L + 0.2 from a guess 0.4 m back")]
    # lost boundary
    s = 40.0
    T["lost"] = [Case(on_track(track, s, n), s, "n = %g" % n) for n in (2.999, 3.001, -2.999, -3.001)]
    for slot, nm in ((3, "vx"), (4, "vy")):
        for v in (99.9, 100.1, -99.9, -100.1):
            c = on_track(track, s, 0.1)
            c[slot] = v
            T["lost"].append(Case(c, s, "%s = %g" % (nm, v)))
    # blown-up states
    T["blown"] = []
    for slot in (5, 6):
        for v in (1e6 - 1, 1e6 + 1, -(1e6 - 1), -(1e6 + 1)):
            c = on_track(track, s, 0.1)
            c[slot] = v
            T["blown"].append(Case(c, s, "cart[%d] = %r" % (slot, v)))
    for slot in range(7):
        for v in (np.nan, np.inf):
            c = on_track(track, s, 0.1)
            c[slot] = v
            T["blown"].append(Case(c, s, "cart[%d] = %r" % (slot, v)))
    T["blown"] += [Case(on_track(track, s, 0.1), g, "guess = %r" % g) for g in (np.nan, np.inf, -np.inf)]
    # reference ramp
    tv = TARGET_VEL
    T["ramp"] = []
    for v, vy, name in [(tv - 1e-9, 0.0, "just below the target"), (tv, 0.0, "at the target"), (tv + 1e-9, 0.0, "just above the target"),
                        (tv - 0.7, 6.0, "cart[3] < target <= hypot(vx, vy)"), (27.5, 0.2, "ramps down"), (0.0, 0.0, "standstill"),
                        (-3.2, 0.1, "negative speed"), (tv - 0.2, 0.0, "clips in the first stage"), (tv + 0.2, 0.0, "clips down in the first stage")]:
        c = on_track(track, 30.0, 0.1, v)
        c[4] = vy
        T["ramp"].append(Case(c, 30.2, name))
    return T


NAMED = ("heading", "newton", "lap", "lost", "blown", "ramp", "circle")     # every case of these tables is a named edge case


def circle_table(track):
    """Eight cars on the circle of laps_numpy.CIRCLE (centre 0, counter-clockwise from angle 0): (cases, s (8,), n (8,)) with the
    closed-form arc length R * angle and offset R - r (left of the driving direction is inside)"""
    R = lp.CIRCLE["radius"]
    ang = np.array([0.3, 1.1, 1.9, 2.7, 3.5, 4.3, 5.1, 5.9])
    r = R + np.array([0.0, 0.4, -0.4, 0.7, -0.7, 0.2, -0.2, 0.5])
    cases = []
    for i in range(8):
        c = np.array([r[i] * np.cos(ang[i]), r[i] * np.sin(ang[i]), ang[i] + np.pi / 2 + 0.05 * (i - 4), 6.1 + 0.25 * i, 0.1, 0.0, 0.02 * (i - 4)])
        cases.append(Case(c, R * ang[i] + 0.5, "angle %.1f radius %.1f" % (ang[i], r[i])))
    return cases, R * ang, R - r


def circle_deviation(track):
    """How far the fitted spline is from the circle, measured on the table at 4000 arc lengths: (largest distance of a point from the
    circle, largest |arc length - R * angle| of a point, largest angle between the spline's tangent and the circle's)"""
    R = lp.CIRCLE["radius"]
    dev = ds = dh = 0.0
    for s in np.linspace(0.0, track.L, 4001)[:-1]:
        x, xd, _ = fn.spline3(track, track.xP, s, np.float64)
        y, yd, _ = fn.spline3(track, track.yP, s, np.float64)
        dev = max(dev, abs(np.hypot(x, y) - R))
        a = np.arctan2(y, x) % (2 * np.pi)
        ds = max(ds, min(abs(R * a - s + k * 2 * np.pi * R) for k in (-1, 0, 1)))
        dh = max(dh, abs(float(fn.angdiff(a + np.pi / 2, np.arctan2(yd, xd), np.float64))))
    return dev, ds, dh


# ---- plant ------------------------------------------------------------------------------------------------------------------------
KP_V, MAX_F, KP_D, MAX_DRATE = 16000.0, 2800.0, 80.0, 0.8        # main.m:84-88
U_LAST_BEFORE = (123.25, -0.375)                                  # what u_last holds before a call: a held car keeps it


def _car(v=V0, vy=0.0, thd=0.0, delta=0.0, theta=0.4):
    return np.array([12.5, -7.25, theta, v, vy, thd, delta])


def plant_tables():
    """name -> list of PlantCase.  exitflag: the car's entry of the flag array (the null-pointer run ignores it); block: index into
    param_blocks() for the run with a parameter block."""
    Z = np.zeros(4)
    T = {}
    rng = np.random.default_rng(9)
    T["ordinary"] = []
    for i in range(32):
        c = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-3, 3), rng.uniform(0, 25), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3),
                      rng.uniform(-0.1, 0.1)])
        near = i % 2 == 0          # every other car inside both actuator limits, the rest as the parity test draws them
        T["ordinary"].append(PlantCase(c, Z, c[3] + rng.uniform(-0.1, 0.1) if near else rng.uniform(0, 25),
                                       c[6] + rng.uniform(-0.005, 0.005) if near else rng.uniform(-0.3, 0.3), 0, 0, 1 + i % 3, "random %d" % i))
    dv, dd = MAX_F / KP_V, MAX_DRATE / KP_D      # 0.175 m/s and 0.01 rad: the errors at which the two outputs reach their limits
    T["pid"] = [
        PlantCase(_car(), Z, V0 + 5.0, 0.0, 0, 0, 0, "force at +PID_MAX_F"),
        PlantCase(_car(), Z, V0 - 5.0, 0.0, 0, 0, 0, "force at -PID_MAX_F"),
        PlantCase(_car(), Z, V0, 0.2, 0, 0, 0, "steering rate at +PID_MAX_DRATE"),
        PlantCase(_car(), Z, V0, -0.2, 0, 0, 0, "steering rate at -PID_MAX_DRATE"),
        PlantCase(_car(), Z, V0 + dv * (1 - 5e-4), 0.0, 0, 0, 0, "force 5e-4 inside +PID_MAX_F"),
        PlantCase(_car(), Z, V0 - dv * (1 + 5e-4), 0.0, 0, 0, 0, "force 5e-4 beyond -PID_MAX_F"),
        PlantCase(_car(), Z, V0, dd * (1 + 5e-4), 0, 0, 0, "steering rate 5e-4 beyond +PID_MAX_DRATE"),
        PlantCase(_car(), Z, V0, -dd * (1 - 5e-4), 0, 0, 0, "steering rate 5e-4 inside -PID_MAX_DRATE"),
        PlantCase(_car(delta=0.05), np.array([3.5, -0.25, 0.125, 0.0625]), V0 + 0.1, 0.055, 0, 0, 0, "carried pid state"),
        PlantCase(_car(delta=0.05), Z, V0 + 0.1, 0.055, 0, 0, 0, "the same car, pid state zero"),
    ]
    T["slip"] = [
        PlantCase(_car(v=0.0), Z, 1.0, 0.1, 0, 0, 0, "standstill"),
        PlantCase(_car(v=-0.01, vy=0.2, thd=0.1), Z, 1.0, 0.1, 0, 0, 0, "x_d = -0.01, atan of an infinity"),
        PlantCase(_car(v=-0.01), Z, 1.0, 0.1, 0, 0, 0, "x_d = -0.01, 0 / 0"),
        PlantCase(_car(v=-5.0, vy=0.1, thd=0.05, delta=0.02), Z, -4.0, 0.0, 0, 0, 0, "reversing"),
    ]
    T["hold"] = [PlantCase(_car(), Z, V0 + 1.0, 0.1, fin, 0, 0, "finished = %d" % fin) for fin in (1, 2)]
    T["hold"] += [PlantCase(_car(), Z, V0 + 1.0, 0.1, 0, f, 0, "exitflag = %d" % f) for f in (-101, -100, -2, -1, 1)]
    T["hold"] += [PlantCase(_car(), Z, np.nan, 0.1, 0, 0, 0, "v_ref = nan"), PlantCase(_car(), Z, V0 + 1.0, np.inf, 0, 0, 0, "delta_ref = inf"),
                  PlantCase(_car(), Z, V0 + 1.0, 0.1, 0, 0, 4, "bad block (with a parameter block only)"),
                  PlantCase(_car(), Z, V0 + 1.0, 0.1, 0, 0, 5, "bad block: negative limit (with a parameter block only)")]
    return T


def param_blocks():
    """(6, 32): 0 the default block; 1 .. 3 other cars; 4: IZ = nan; 5: PID_MAX_F < 0.  A table's cars index it (PlantCase.block), which
    gives the per-car (B, 32) array of the call."""
    rng = np.random.default_rng(41)
    P = np.tile(default_block(1), (6, 1))
    for i in (1, 2, 3):
        for name in ("M", "IZ", "LF", "LR", "PB", "PC", "PD", "PE", "PID_KP_V", "PID_MAX_F", "PID_KP_D", "PID_MAX_DRATE"):
            P[i, pn.IDX[name]] *= 1 + rng.uniform(-0.15, 0.15)
    P[4, pn.IDX["IZ"]] = np.nan
    P[5, pn.IDX["PID_MAX_F"]] = -1.0
    return P


# ---- accept -------------------------------------------------------------------------------------------------------------------------
def accept_table(nx, N):
    """dict: x_new (B, N nx), u_new (B, 2 N), x_keep, u_keep, exitflag (B,) int32, name.  Flags 0 and 1 take over; -1, -2, -3, 2 and 4 do
    not; one NaN or Inf at the first, a middle and the last entry of x_new and of u_new, one at a time, under flag 0."""
    lx, lu = nx * N, 2 * N
    rows = [(f, None, None, None, "flag %d" % f) for f in (0, 1, -1, -2, -3, 2, 4)]
    for which, n in (("x", lx), ("u", lu)):
        for pos in (0, n // 2, n - 1):
            for bad in (np.nan, np.inf, -np.inf):
                rows.append((0, which, pos, bad, "%r at %s_new[%d]" % (bad, which, pos)))
    B = len(rows)
    rng = np.random.default_rng(5)
    t = dict(x_new=rng.uniform(-1, 1, (B, lx)), u_new=rng.uniform(-1, 1, (B, lu)), x_keep=rng.uniform(2, 3, (B, lx)), u_keep=rng.uniform(2, 3, (B, lu)),
             exitflag=np.array([r[0] for r in rows], dtype=np.int32), name=[r[4] for r in rows])
    for b, (_, which, pos, bad, _) in enumerate(rows):
        if which is not None:
            t[which + "_new"][b, pos] = bad
    return t


# ---- the references: both dtypes of the restatement, the drop rule, e64 and the tolerance of a table -----------------------------------
LD = np.longdouble


def x0_error(got, ref):
    """|got - ref| entry by entry for (B, nx) frame states, as long doubles.  The heading error (column 2) is taken on the circle: at
    a heading exactly opposite to the track +pi and -pi are one angle, and the last bit of atan2 picks the name."""
    e = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    e[:, 2] = np.minimum(e[:, 2], np.abs(e[:, 2] - 2 * LD(np.pi)))
    return e


def _worst(e, keep):
    e = np.asarray(e)[keep]
    e = e[np.isfinite(e.astype(np.float64))]
    return float(e.max()) if e.size else 0.0


def frame_reference(track, cases, model, N, target_vel):
    """The restatement on a frame table in both dtypes.  dict: x0 (B, nx), x_ref (B, N, nx), finished (B,) of the long-double run;
    x0_64, x_ref_64 of the float64 run; newton (B,); dropped (B,) bool: the two runs disagree on a discrete outcome (Newton steps,
    finished, the side of the ramp's clip in a stage); e64 and tol per tensor over the cars that stay."""
    out = {k: [] for k in ("x0", "x_ref", "finished", "x0_64", "x_ref_64", "newton", "dropped")}
    for c in cases:
        i64, i80 = {}, {}
        a = fn.pre(model, N, DT, target_vel, track, c.cart, c.guess, np.float64, i64)
        b = fn.pre(model, N, DT, target_vel, track, c.cart, c.guess, LD, i80)
        out["x0"].append(b[0]); out["x_ref"].append(b[1]); out["finished"].append(b[2])
        out["x0_64"].append(a[0]); out["x_ref_64"].append(a[1]); out["newton"].append(i80["newton"])
        out["dropped"].append(i64 != i80)
    out = {k: np.array(v) for k, v in out.items()}
    keep = ~out["dropped"]
    out["e64"] = dict(x0=_worst(x0_error(out["x0_64"], out["x0"]), keep), x_ref=_worst(np.abs(out["x_ref_64"] - out["x_ref"]), keep))
    out["tol"] = {k: tolerance(out["e64"][k], out[k][keep]) for k in ("x0", "x_ref")}
    return out


def plant_reference(cases, blocks=None, null_flags=False):
    """The restatement on a plant table in both dtypes (blocks: param_blocks() or None = the compiled-in constants; null_flags: the
    call passes no flag array).  dict: cart (B, 7), pid (B, 4), u_last (B, 2), held (B,) of the long-double run, *_64 of the float64
    run, dropped (B,): the runs disagree on the saturated side of a PID in a sub-step; e64 and tol per tensor over finite entries."""
    names = ("cart", "pid", "u_last")
    out = {k: [] for k in names + tuple(n + "_64" for n in names) + ("held", "dropped")}
    for c in cases:
        blk = None if blocks is None else blocks[c.block]
        bad = blk is not None and fn.block_is_bad(blk)
        flag = None if null_flags else c.exitflag
        i64, i80 = {}, {}
        a = fn.plant(blk, c.cart, c.pid, U_LAST_BEFORE, c.v_ref, c.delta_ref, DT, c.finished, flag, bad, np.float64, i64)
        b = fn.plant(blk, c.cart, c.pid, U_LAST_BEFORE, c.v_ref, c.delta_ref, DT, c.finished, flag, bad, LD, i80)
        for j, n in enumerate(names):
            out[n].append(b[j]); out[n + "_64"].append(a[j])
        out["held"].append(b[3]); out["dropped"].append(i64 != i80)
    out = {k: np.array(v) for k, v in out.items()}
    keep = ~out["dropped"]
    with np.errstate(invalid="ignore"):
        out["e64"] = {n: _worst(np.abs(out[n + "_64"] - out[n]), keep) for n in names}
    out["tol"] = {n: tolerance(out["e64"][n], out[n][keep]) for n in names}
    return out


def same_finite_pattern(got, ref):
    """a reference entry that is not finite asks for a non-finite entry of the result (a NaN may come back as an Inf), and nothing else may be non-finite"""
    return bool(np.array_equal(np.isfinite(np.asarray(got, dtype=np.float64)), np.isfinite(np.asarray(ref, dtype=np.float64))))


def finite_error(got, ref):
    """largest |got - ref| over the finite entries of ref, as a float"""
    ref = np.asarray(ref, dtype=LD)
    fin = np.isfinite(ref.astype(np.float64))
    with np.errstate(invalid="ignore"):
        e = np.abs(np.asarray(got, dtype=LD) - ref)[fin]
    return float(e.max()) if e.size else 0.0
